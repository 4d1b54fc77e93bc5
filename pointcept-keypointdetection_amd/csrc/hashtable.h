// Open-addressing table of active sites (batch, x, y, z) -> row: key / probe functions shared by the submanifold
// neighbour search (sparse.hip) and the cell-grid kNN (pointops.hip).  Layout of a table of `slots` entries:
// slots x uint64 keys, then slots x int32 values.
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>

namespace ptv3 {

constexpr uint64_t HT_EMPTY = ~0ull;

__device__ __forceinline__ uint64_t site_key(int b, int x, int y, int z) {
  return ((uint64_t)(uint32_t)b << 48) | ((uint64_t)(uint32_t)x << 32) | ((uint64_t)(uint32_t)y << 16) |
         (uint64_t)(uint32_t)z;
}
__device__ __forceinline__ uint64_t mix64(uint64_t k) {
  k ^= k >> 33; k *= 0xff51afd7ed558ccdull; k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ull; k ^= k >> 33;
  return k;
}
// row of site (b, x, y, z), or -1
__device__ __forceinline__ int32_t ht_find(const unsigned long long* __restrict__ keys,
                                           const int32_t* __restrict__ vals, uint64_t mask, int b, int x, int y, int z) {
  if (x < 0 || y < 0 || z < 0 || x >= 65536 || y >= 65536 || z >= 65536) return -1;
  const uint64_t key = site_key(b, x, y, z);
  uint64_t slot = mix64(key) & mask;
  for (uint64_t probe = 0; probe <= mask; ++probe) {
    const unsigned long long kq = keys[slot];
    if (kq == key) return vals[slot];
    if (kq == HT_EMPTY) return -1;
    slot = (slot + 1) & mask;
  }
  return -1;
}

// ---- block table: open addressing over 4 x 4 x 4 blocks of sites -------------------------------------------------
// A 32-byte slot holds everything a lookup of one block needs, so the 64 voxels of a block share one line where the
// per-voxel table above spends a line per probed voxel.  key = site_key(b, x>>2, y>>2, z>>2) | BT_USED (batch < 32768
// leaves bit 63 free, so a zero-filled table is an empty one); mask bit ((x&3)<<4)|((y&3)<<2)|(z&3) = voxel occupied;
// the rows of the occupied voxels, in bit order, are payload[base .. base + popcount(mask)).
struct alignas(16) BlockSlot {
  unsigned long long key;
  unsigned long long mask;
  int32_t base;
  int32_t pad_[3];
};
constexpr uint64_t BT_USED = 1ull << 63;

__device__ __forceinline__ uint64_t block_key(int b, int bx, int by, int bz) { return site_key(b, bx, by, bz) | BT_USED; }
__device__ __forceinline__ int block_bit(int x, int y, int z) { return ((x & 3) << 4) | ((y & 3) << 2) | (z & 3); }
// slot of block (b, bx, by, bz), or -1; block coordinates in [0, 16384)
__device__ __forceinline__ int64_t bt_find(const BlockSlot* __restrict__ slots, uint64_t smask, int b, int bx, int by,
                                           int bz) {
  const uint64_t key = block_key(b, bx, by, bz);
  uint64_t slot = mix64(key) & smask;
  for (uint64_t probe = 0; probe <= smask; ++probe) {
    const unsigned long long kq = slots[slot].key;
    if (kq == key) return (int64_t)slot;
    if (kq == 0) return -1;
    slot = (slot + 1) & smask;
  }
  return -1;
}

}  // namespace ptv3
