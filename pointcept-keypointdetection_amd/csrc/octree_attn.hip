// OctFormer (pointcept/models/octformer/octformer_v1m1_base.py) on gfx950: the leaf keys of the octree, the octree
// attention between the qkv and proj linears (:224-262) and the block's conditional positional encoding (:143-160, :310).
//
// ptv3_octree_attn_fwd: one wave per (patch, head).  A patch is K <= 32 tokens: token j of patch d of group g is node
// row g*K*D + j*D + d, which is the reference's patch_partition + view(-1, K, D, C).transpose(1, 2) without the padded
// copy.  The wave stages the patch's k and v rows of its head, the token coordinates and scene ids and the head's
// column of the RPE table in LDS; lane (r, half) = (lane & 31, lane >> 5) then holds query r in registers and walks the
// 16 keys of its half (every lane of a half reads the same LDS address: a broadcast, no bank conflict).  The two halves
// meet in three cross-lane exchanges (row maximum, row sum, the output row).  All arithmetic is fp32 fused multiply-add
// in a fixed order: the result is bitwise reproducible, there is no atomic and every store is a 16-byte vector store.
//
// Keys of another scene, and the padding rows at or past n_t (scene id batch_size in the reference), carry -1e3 in the
// reference.  With logits of ordinary size exp() of that is 0 in fp32, so the kernel SKIPS those keys instead of adding
// -1e3: a query attends to the keys of its own scene inside its patch, of which it is always one.  Rows at or past n_t
// are never read and never written.
#include "common.h"
#include "../../include/ptv3_hip.h"

namespace ptv3 {
namespace {

constexpr int OCT_MAX_K = 32;        // tokens per patch the wave holds
constexpr int OCT_MAX_BND = 127;     // pos_bnd: 3 * (2 * 127 + 1) table entries of one head in LDS
constexpr int OCT_MAX_DEPTH = 16;    // 3 * 16 key bits under the scene id at bit 48

__device__ __forceinline__ unsigned long long spread3(unsigned v) {
  // bit i of v -> bit 3 i
  unsigned long long x = v & 0xffffu;
  x = (x | (x << 32)) & 0x1f00000000ffffull;
  x = (x | (x << 16)) & 0x1f0000ff0000ffull;
  x = (x | (x << 8)) & 0x100f00f00f00f00full;
  x = (x | (x << 4)) & 0x10c30c30c30c30c3ull;
  x = (x | (x << 2)) & 0x1249249249249249ull;
  return x;
}

// cell = floor((coord / scale_factor + 1) * 2^(depth-1)) in fp32, one rounding per operation (IEEE division), as torch
// evaluates it; a point outside -1 <= p < 1 (NaN included) raises the flag and is clamped into the grid.
__global__ void octree_keys_kernel(const float* __restrict__ coord, const int32_t* __restrict__ offset, int num_scenes,
                                   int64_t n, float scale_factor, int depth, int64_t* __restrict__ key,
                                   int32_t* __restrict__ flag) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int lo = 0, hi = num_scenes - 1;   // first scene whose end lies past i
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if ((int64_t)offset[mid] > i) hi = mid; else lo = mid + 1;
  }
  const float half = (float)(1u << (depth - 1));
  const int top = (1 << depth) - 1;
  unsigned cell[3];
  bool bad = false;
  for (int a = 0; a < 3; ++a) {
    const float p = __fdiv_rn(coord[i * 3 + a], scale_factor);
    bad |= !(p >= -1.0f && p < 1.0f);
    const float f = floorf(__fmul_rn(__fadd_rn(p, 1.0f), half));
    int c = (f >= 0.0f) ? (f <= (float)top ? (int)f : top) : 0;
    cell[a] = (unsigned)c;
  }
  if (bad) *flag = 1;   // every writer stores the same value
  key[i] = (int64_t)(((unsigned long long)lo << 48) | (spread3(cell[0]) << 2) | (spread3(cell[1]) << 1) |
                     spread3(cell[2]));
}

template <int HD>
__global__ __launch_bounds__(64) void octree_attn_kernel(const float* __restrict__ qkv, const int32_t* __restrict__ xyz,
                                                         const int32_t* __restrict__ batch,
                                                         const float* __restrict__ table, float* __restrict__ out,
                                                         int64_t n_t, int c, int heads, int patch, int dilation,
                                                         int pos_bnd, float scale) {
  __shared__ __attribute__((aligned(16))) float ks[OCT_MAX_K][HD];
  __shared__ __attribute__((aligned(16))) float vs[OCT_MAX_K][HD];
  __shared__ int sx[OCT_MAX_K], sy[OCT_MAX_K], sz[OCT_MAX_K], sb[OCT_MAX_K];
  __shared__ float tab[3 * (2 * OCT_MAX_BND + 1)];

  const int lane = threadIdx.x;
  const int h = blockIdx.y;
  const int64_t g = blockIdx.x / dilation;
  const int d = blockIdx.x % dilation;
  const int64_t row0 = g * (int64_t)patch * dilation + d;
  const int rpe_num = 2 * pos_bnd + 1;
  const int64_t ld = 3 * (int64_t)c;

  for (int i = lane; i < 3 * rpe_num; i += 64) tab[i] = table[(int64_t)i * heads + h];
  if (lane < OCT_MAX_K) {
    const int64_t row = row0 + (int64_t)lane * dilation;
    const bool ok = lane < patch && row < n_t;
    sx[lane] = ok ? xyz[row * 3 + 0] : 0;
    sy[lane] = ok ? xyz[row * 3 + 1] : 0;
    sz[lane] = ok ? xyz[row * 3 + 2] : 0;
    sb[lane] = ok ? batch[row] : -1;   // -1 matches no query: a skipped key
  }
  constexpr int V = HD / 4;   // float4 per row of one head
  for (int i = lane; i < OCT_MAX_K * V; i += 64) {
    const int t = i / V, p = i % V;
    const int64_t row = row0 + (int64_t)t * dilation;
    f32x4 kk = f32x4{0.f, 0.f, 0.f, 0.f}, vv = kk;
    if (t < patch && row < n_t) {
      const float* base = qkv + row * ld + (int64_t)h * HD + p * 4;
      kk = *reinterpret_cast<const f32x4*>(base + c);
      vv = *reinterpret_cast<const f32x4*>(base + 2 * (int64_t)c);
    }
    *reinterpret_cast<f32x4*>(&ks[t][p * 4]) = kk;
    *reinterpret_cast<f32x4*>(&vs[t][p * 4]) = vv;
  }
  __syncthreads();

  const int r = lane & 31, half = lane >> 5;
  const int64_t qrow = row0 + (int64_t)r * dilation;
  const bool qok = r < patch && qrow < n_t;
  float q[HD];
  if (qok) {
    const float* base = qkv + qrow * ld + (int64_t)h * HD;
#pragma unroll
    for (int p = 0; p < V; ++p) {
      const f32x4 t = *reinterpret_cast<const f32x4*>(base + p * 4);
      q[p * 4 + 0] = t[0] * scale; q[p * 4 + 1] = t[1] * scale; q[p * 4 + 2] = t[2] * scale; q[p * 4 + 3] = t[3] * scale;
    }
  } else {
#pragma unroll
    for (int p = 0; p < HD; ++p) q[p] = 0.f;
  }
  const int qx = sx[r], qy = sy[r], qz = sz[r];
  const int qb = qok ? sb[r] : -2;

  float s[16];
  float m = -INFINITY;
#pragma unroll
  for (int jj = 0; jj < 16; ++jj) {
    const int j = half * 16 + jj;
    float acc = 0.f;
#pragma unroll
    for (int p = 0; p < V; ++p) {
      const f32x4 kk = *reinterpret_cast<const f32x4*>(&ks[j][p * 4]);
      acc = fmaf(q[p * 4 + 0], kk[0], acc);
      acc = fmaf(q[p * 4 + 1], kk[1], acc);
      acc = fmaf(q[p * 4 + 2], kk[2], acc);
      acc = fmaf(q[p * 4 + 3], kk[3], acc);
    }
    const int dx = min(max(qx - sx[j], -pos_bnd), pos_bnd) + pos_bnd;
    const int dy = min(max(qy - sy[j], -pos_bnd), pos_bnd) + pos_bnd + rpe_num;
    const int dz = min(max(qz - sz[j], -pos_bnd), pos_bnd) + pos_bnd + 2 * rpe_num;
    const float bias = (tab[dx] + tab[dy]) + tab[dz];
    s[jj] = (sb[j] == qb) ? acc + bias : -INFINITY;
    m = fmaxf(m, s[jj]);
  }
  m = fmaxf(m, __shfl_xor(m, 32));

  float o[HD];
#pragma unroll
  for (int p = 0; p < HD; ++p) o[p] = 0.f;
  float l = 0.f;
#pragma unroll
  for (int jj = 0; jj < 16; ++jj) {
    const int j = half * 16 + jj;
    const float pj = (s[jj] == -INFINITY) ? 0.f : expf(s[jj] - m);
    l += pj;
#pragma unroll
    for (int p = 0; p < V; ++p) {
      const f32x4 vv = *reinterpret_cast<const f32x4*>(&vs[j][p * 4]);
      o[p * 4 + 0] = fmaf(pj, vv[0], o[p * 4 + 0]);
      o[p * 4 + 1] = fmaf(pj, vv[1], o[p * 4 + 1]);
      o[p * 4 + 2] = fmaf(pj, vv[2], o[p * 4 + 2]);
      o[p * 4 + 3] = fmaf(pj, vv[3], o[p * 4 + 3]);
    }
  }
  // a + b is commutative, so both halves hold the same bits after the exchange
  l += __shfl_xor(l, 32);
#pragma unroll
  for (int p = 0; p < HD; ++p) o[p] += __shfl_xor(o[p], 32);
  if (!qok) return;
  // l >= exp(0) of the row's maximum: the query's own key is never skipped
  float* dst = out + qrow * (int64_t)c + (int64_t)h * HD + half * (HD / 2);
#pragma unroll
  for (int p = 0; p < V / 2; ++p) {
    f32x4 w;
#pragma unroll
    for (int e = 0; e < 4; ++e) w[e] = __fdiv_rn(half ? o[HD / 2 + p * 4 + e] : o[p * 4 + e], l);
    *reinterpret_cast<f32x4*>(dst + p * 4) = w;
  }
}

// out = x + (sum_t w[t][c] x[nbr[i][t]][c]) * bn_scale[c] + bn_shift[c]; one thread per (row, 4 channels)
__global__ void octree_dwconv_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                     const int32_t* __restrict__ nbr, const float* __restrict__ bn_scale,
                                     const float* __restrict__ bn_shift, float* __restrict__ out, int64_t n, int c) {
  const int v = c >> 2;
  const int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= n * v) return;
  const int64_t i = id / v;
  const int p = (int)(id % v) * 4;
  f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
  const int32_t* nb = nbr + i * 27;
#pragma unroll 9
  for (int t = 0; t < 27; ++t) {
    const int32_t j = nb[t];
    if ((uint32_t)j >= (uint64_t)n) continue;   // -1 (or anything outside [0, n)): an absent tap
    const f32x4 xv = *reinterpret_cast<const f32x4*>(x + (int64_t)j * c + p);
    const f32x4 wv = *reinterpret_cast<const f32x4*>(w + (int64_t)t * c + p);
    acc[0] = fmaf(wv[0], xv[0], acc[0]); acc[1] = fmaf(wv[1], xv[1], acc[1]);
    acc[2] = fmaf(wv[2], xv[2], acc[2]); acc[3] = fmaf(wv[3], xv[3], acc[3]);
  }
  const f32x4 xi = *reinterpret_cast<const f32x4*>(x + i * c + p);
  const f32x4 sc = *reinterpret_cast<const f32x4*>(bn_scale + p);
  const f32x4 sh = *reinterpret_cast<const f32x4*>(bn_shift + p);
  f32x4 y;
#pragma unroll
  for (int e = 0; e < 4; ++e) y[e] = xi[e] + fmaf(acc[e], sc[e], sh[e]);
  *reinterpret_cast<f32x4*>(out + i * c + p) = y;
}

}  // namespace
}  // namespace ptv3

using namespace ptv3;

extern "C" int ptv3_octree_keys(const float* coord, const int32_t* offset, int num_scenes, int64_t n, float scale_factor,
                                int depth, int64_t* key, int32_t* flag, void* stream) {
  PTV3_REQUIRE(coord && offset && key && flag, "octree_keys: null pointer");
  PTV3_REQUIRE(n >= 1 && n < ((int64_t)1 << 31), "octree_keys: n = %lld out of [1, 2^31)", (long long)n);
  PTV3_REQUIRE(num_scenes >= 1 && num_scenes < 32768, "octree_keys: %d scenes out of [1, 32768)", num_scenes);
  PTV3_REQUIRE(depth >= 1 && depth <= OCT_MAX_DEPTH, "octree_keys: depth %d out of [1, %d]", depth, OCT_MAX_DEPTH);
  PTV3_REQUIRE(scale_factor > 0.f, "octree_keys: scale factor must be positive");
  hipLaunchKernelGGL(octree_keys_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, coord, offset,
                     num_scenes, n, scale_factor, depth, key, flag);
  PTV3_LAUNCH_CHECK();
  return PTV3_OK;
}

extern "C" int ptv3_octree_attn_capable(int c, int heads, int patch, int dilation) {
  if (heads < 1 || c < 1 || c % heads) return 0;
  const int hd = c / heads;
  return (hd == 16 || hd == 32) && patch >= 1 && patch <= OCT_MAX_K && dilation >= 1 && heads <= 65535;
}

extern "C" int ptv3_octree_attn_fwd(const float* qkv, const int32_t* xyz, const int32_t* batch, const float* rpe_table,
                                    float* out, int64_t n_t, int c, int heads, int patch, int dilation, int pos_bnd,
                                    float scale, void* stream) {
  PTV3_REQUIRE(qkv && xyz && batch && rpe_table && out, "octree_attn: null pointer");
  PTV3_REQUIRE(n_t >= 1 && n_t < ((int64_t)1 << 31), "octree_attn: n_t = %lld out of [1, 2^31)", (long long)n_t);
  PTV3_REQUIRE(c >= 1 && heads >= 1 && patch >= 1 && dilation >= 1 && pos_bnd >= 0,
               "octree_attn: c %d, heads %d, patch %d, dilation %d, pos_bnd %d must be positive", c, heads, patch,
               dilation, pos_bnd);
  PTV3_REQUIRE(c % heads == 0, "octree_attn: %d channels do not divide into %d heads", c, heads);
  if (!ptv3_octree_attn_capable(c, heads, patch, dilation) || pos_bnd > OCT_MAX_BND) {
    set_error("octree_attn: head dimension %d (16 or 32), patch %d (<= %d) or pos_bnd %d (<= %d) not covered", c / heads,
              patch, OCT_MAX_K, pos_bnd, OCT_MAX_BND);
    return PTV3_ERR_UNSUPPORTED;
  }
  const int64_t groups = cdiv(n_t, (int64_t)patch * dilation);
  const int64_t patches = groups * dilation;
  PTV3_REQUIRE(patches < ((int64_t)1 << 31), "octree_attn: %lld patches", (long long)patches);
  const dim3 grid((unsigned)patches, (unsigned)heads);
  if (c / heads == 16)
    hipLaunchKernelGGL(octree_attn_kernel<16>, grid, dim3(64), 0, (hipStream_t)stream, qkv, xyz, batch, rpe_table, out,
                       n_t, c, heads, patch, dilation, pos_bnd, scale);
  else
    hipLaunchKernelGGL(octree_attn_kernel<32>, grid, dim3(64), 0, (hipStream_t)stream, qkv, xyz, batch, rpe_table, out,
                       n_t, c, heads, patch, dilation, pos_bnd, scale);
  PTV3_LAUNCH_CHECK();
  return PTV3_OK;
}

extern "C" int ptv3_octree_dwconv(const float* x, const float* w, const int32_t* nbr, const float* bn_scale,
                                  const float* bn_shift, float* out, int64_t n, int c, void* stream) {
  PTV3_REQUIRE(x && w && nbr && bn_scale && bn_shift && out, "octree_dwconv: null pointer");
  PTV3_REQUIRE(n >= 1 && n < ((int64_t)1 << 31), "octree_dwconv: n = %lld out of [1, 2^31)", (long long)n);
  PTV3_REQUIRE(c >= 4 && c % 4 == 0 && c <= 4096, "octree_dwconv: %d channels (a multiple of 4 up to 4096)", c);
  PTV3_REQUIRE(x != out, "octree_dwconv: out must not alias x (neighbours read x)");
  const int64_t threads = n * (c / 4);
  PTV3_REQUIRE(cdiv(threads, 256) < ((int64_t)1 << 31), "octree_dwconv: %lld x %d is too large for one launch", (long long)n, c);
  hipLaunchKernelGGL(octree_dwconv_kernel, dim3((unsigned)cdiv(threads, 256)), dim3(256), 0, (hipStream_t)stream, x, w,
                     nbr, bn_scale, bn_shift, out, n, c);
  PTV3_LAUNCH_CHECK();
  return PTV3_OK;
}
