/* ptv3_hip.h -- C ABI of libptv3_hip.so: the MI355X (gfx950) kernels behind the PTv3
 * serialized-window attention path of Pointcept-KeypointDetection.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the name ends in _host;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); every call only enqueues
 *     work on that stream: no allocation, no synchronisation, graph-capturable;
 *   - `dtype`: PTV3_F32 (0) = fp32 storage, exact-fp32 matrix-core math (parity mode);
 *              PTV3_BF16 (1) = bf16 storage, bf16 MFMA with fp32 accumulate / fp32 softmax+norm;
 *   - return value: 0 on success, non-zero on error (ptv3_last_error() gives the message);
 *   - tensors are dense row-major.  "rows" of feature matrices are points.
 *
 * Each entry point names the reference interface it replaces (paths relative to the reference
 * repository root).  The Python binding a maintainer adds is in INTEGRATION.md.
 */
#ifndef PTV3_HIP_H
#define PTV3_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PTV3_F32 0
#define PTV3_BF16 1

/* return codes */
#define PTV3_OK 0
#define PTV3_ERR_ARG 1         /* a malformed call */
#define PTV3_ERR_LAUNCH 2      /* a kernel launch failed */         
#define PTV3_ERR_UNSUPPORTED 3 /* a well-formed shape no kernel serves */

/* curve ids for ptv3_sfc_encode (pointcept/models/utils/serialization/default.py:9-24) */
#define PTV3_ORDER_Z 0
#define PTV3_ORDER_Z_TRANS 1
#define PTV3_ORDER_HILBERT 2
#define PTV3_ORDER_HILBERT_TRANS 3

/* epilogue activation ids for ptv3_gemm */
#define PTV3_ACT_NONE 0
#define PTV3_ACT_GELU 1 /* erf form = torch.nn.GELU() default */
#define PTV3_ACT_RELU 2

const char* ptv3_last_error(void);
int ptv3_version(void);

/* ---- serialization ------------------------------------------------------------------------
 * replaces encode() (utils/serialization/default.py:9-24), z_order.xyz2key (z_order.py:66-101)
 * and hilbert.encode (hilbert.py:91-198): code[r][i] = batch[i] << 3*depth | curve_r(grid_coord[i]).
 * grid_coord: (n,3) int32 (coord_is_i64=0) or int64 (=1); batch: (n) int64 or NULL;
 * order_ids_host: k curve ids (host array); code: (k,n) int64. */
int ptv3_sfc_encode(const void* grid_coord, int coord_is_i64, const int64_t* batch, int64_t n,
                    int depth, const int* order_ids_host, int k, int64_t* code, void* stream);

/* replaces torch.argsort + scatter_ of arange in Point.serialization
 * (models/utils/structure.py:92-99) and SerializedPooling (point_transformer_v3m1_base.py:399-406):
 * per row r: order[r] = stable argsort(code[r]); inverse[r][order[r][i]] = i.
 * code: (k,n) int64 compared as UNSIGNED 64-bit with all set bits below `end_bit` (<= 64; serialization codes
 * are non-negative, the GridSample voxel hashes use all 64 bits); order/inverse: (k,n) int64.
 * workspace: ptv3_argsort_workspace_bytes(k,n) bytes. */
size_t ptv3_argsort_workspace_bytes(int k, int64_t n);
int ptv3_argsort_i64(const int64_t* code, int k, int64_t n, int end_bit, int64_t* order,
                     int64_t* inverse, void* workspace, size_t workspace_bytes, void* stream);

/* The executor's form of ptv3_argsort_i64, order and inverse bit for bit the same.
 * row_order (optional, NULL = skip): (n) int32, row 0 of `order` once more: the gather order of the sparse
 * convolutions, written by the last pass.  ptv3_argsort_scan_batch: per-block counters a scatter workgroup loads per
 * round trip when it derives its own digit bases (the sizes on both sides of a multiple of it x 2048 keys take
 * different trips). */
int ptv3_argsort_i64_rows(const int64_t* code, int k, int64_t n, int end_bit, int64_t* order, int64_t* inverse,
                          int32_t* row_order, void* workspace, size_t workspace_bytes, void* stream);
int ptv3_argsort_scan_batch(void);

/* max(0, largest of the 3n grid coordinates) -> out_max[0] (int32, device or pinned host memory):
 * serialization depth = bit_length(max + 1) (models/utils/structure.py:73).  int64 coordinates are read as int32.
 * state: two device int32 that are zero before the call; the call leaves them zero again (one launch, no fill). */
int ptv3_coord_max(const void* grid_coord, int coord_is_i64, int64_t n, int32_t* state, int32_t* out_max, void* stream);

/* ---- patch partition ----------------------------------------------------------------------
 * replaces SerializedAttention.get_padding_and_inverse (point_transformer_v3m1_base.py:114-170).
 * offset: (b) int64 cumulative scene ends (device); patch = K.  A scene of n_b > K points is padded to a
 * multiple of K (pad-by-borrowing, :144-154) and cut into K-slot windows; a scene of n_b <= K points stays
 * ONE window of n_b slots (:131-133 - only reachable with enable_flash=True, where K is fixed; with
 * enable_flash=False K = min(smallest scene, patch) and every window has K slots).
 * n_pad = sum_b (n_b > K ? ceil_to_K(n_b) : n_b);  windows = sum_b ceil(n_b / K).
 * pad: (n_pad) int64, unpad: (n) int64, cu_seqlens: (windows + 1) int32 window starts + n_pad. */
int ptv3_pad_plan(const int64_t* offset, int b, int64_t n, int64_t n_pad, int patch, int64_t* pad,
                  int64_t* unpad, int32_t* cu_seqlens, void* stream);

/* composes the two gathers of SerializedAttention.forward (point_transformer_v3m1_base.py:184-185):
 * win_order[p] = order[pad[p]] (n_pad), win_inverse[i] = unpad[inverse[i]] (n); int32 outputs. */
int ptv3_window_maps(const int64_t* order, const int64_t* inverse, const int64_t* pad,
                     const int64_t* unpad, int64_t n, int64_t n_pad, int32_t* win_order,
                     int32_t* win_inverse, void* stream);

/* pad plan + both maps for all k orders in one launch (no pad / unpad materialised): the executor's form of
 * the two entry points above.  order / inverse: (k, n); win_order: (k, n_pad); win_inverse: (k, n);
 * cu_seqlens (optional, NULL = skip): (windows + 1) int32 as ptv3_pad_plan writes it. */
int ptv3_window_plan(const int64_t* order, const int64_t* inverse, const int64_t* offset, int b, int k,
                     int64_t n, int64_t n_pad, int patch, int32_t* win_order, int32_t* win_inverse,
                     int32_t* cu_seqlens, void* stream);

/* ---- window attention ----------------------------------------------------------------------
 * replaces the vanilla branch of SerializedAttention.forward (point_transformer_v3m1_base.py:188-216)
 * = what flash_attn_varlen_qkvpacked_func computes on the reference's CUDA path (:208-214):
 *   x = qkv[win_order]; per window of `patch` rows and head h:
 *   out_w = softmax(scale * q k^T) v;  out[i] = concat_h(out_w)[win_inverse[i]].
 * qkv: (n, 3*c) with channel layout [3][heads][c/heads]; out: (n, c).  c/heads must be 16, 32 or 64.
 * rpe_bias (optional, may be NULL): (n_pad/patch, heads, patch, patch) fp32 added to the scores
 * (RPE.forward, :29-48). */
int ptv3_window_attn_fwd(const void* qkv, const int32_t* win_order, const int32_t* win_inverse,
                         void* out, int64_t n, int64_t n_pad, int c, int heads, int patch, float scale,
                         const float* rpe_bias, int dtype, void* stream);

/* The enable_flash=True form of the same attention: what flash_attn_varlen_qkvpacked_func(qkv[order], cu_seqlens,
 * max_seqlen=K, softmax_scale) computes at the reference's call site (point_transformer_v3m1_base.py:207-215;
 * flash-attn 2.6.3 is a CUDA-only wheel outside the reference tree - its published semantics are restated:
 * independent softmax(scale q k^T) v per sequence [cu_seqlens[w], cu_seqlens[w+1]) and head).  Windows may be
 * ragged: window w holds the padded slots [cu_seqlens[w], cu_seqlens[w+1]), 1..max_seqlen of them (a scene with
 * fewer than K points is one short window, :131-133).  cu_seqlens: (num_windows + 1) int32, device, as
 * ptv3_pad_plan / ptv3_window_plan write it.  sum_len_sq (host, measurement only): sum over windows of len^2
 * for the algorithmic flop count, 0 = unknown (n_pad * max_seqlen is used).  Arithmetic follows `dtype` like
 * ptv3_window_attn_fwd (the reference casts qkv to bf16 for flash-attn whatever the model dtype, :209). */
int ptv3_window_attn_varlen_fwd(const void* qkv, const int32_t* win_order, const int32_t* win_inverse,
                                const int32_t* cu_seqlens, int num_windows, void* out, int64_t n, int64_t n_pad,
                                int c, int heads, int max_seqlen, float scale, double sum_len_sq, int dtype,
                                void* stream);

/* Same attention with the relative-position bias of RPE (point_transformer_v3m1_base.py:29-48 applied to
 * get_rel_pos :104-112) evaluated INSIDE the kernel: bias(q, k, h) = sum over the 3 axes of
 * rpe_table[axis * (2*pos_bnd+1) + clamp(grid[q][axis] - grid[k][axis], -pos_bnd, pos_bnd) + pos_bnd][h],
 * from the window's voxel coordinates and the head's table column held in LDS - the (windows, H, K, K) bias
 * tensor of the rpe_bias argument above (3.3 GB per call at 100k points, K = 1024) is never built.
 * grid_coord (n, 3) int32 in point order; rpe_table (3*(2*pos_bnd+1), heads) fp32.  PTV3_ERR_UNSUPPORTED when the
 * window does not fit the resident-window kernel (then build the dense bias and use ptv3_window_attn_fwd). */
int ptv3_window_attn_rpe_fwd(const void* qkv, const int32_t* win_order, const int32_t* win_inverse, void* out,
                             int64_t n, int64_t n_pad, int c, int heads, int patch, float scale,
                             const int32_t* grid_coord, const float* rpe_table, int pos_bnd, int dtype,
                             void* stream);

/* ---- sparse submanifold convolution + dense linear (one implicit-GEMM kernel) ---------------
 * Hash of the active sites: replaces spconv's indice-pair generation behind
 * spconv.SparseConvTensor / SubMConv3d(indice_key=...) (models/utils/structure.py:111-146,
 * point_transformer_v3m1_base.py:277-284,499-506).
 * indices: (n,4) int32 [batch,x,y,z] unique rows, 0 <= x,y,z < 65536, batch < 32768.
 * table: `slots` int64 keys + `slots` int32 values, slots = power of two >= 2n
 * (ptv3_subm_table_slots(n)); layout: keys first.  nbr: (n, kvol) int32, -1 = inactive;
 * kernel offset index (a,b,c) -> a*k*k + b*k + c pairs with (x+a-k/2, y+b-k/2, z+c-k/2). */
int64_t ptv3_subm_table_slots(int64_t n);
int ptv3_subm_build_table(const int32_t* indices, int64_t n, void* table, int64_t slots, void* stream);
int ptv3_subm_neighbors(const int32_t* indices, int64_t n, const void* table, int64_t slots, int ksize,
                        int32_t* nbr, void* stream);

/* The same neighbour table (bitwise the one the full-probing form of ptv3_subm_neighbors gives, duplicate rows
 * included: the smallest row of a coordinate wins, the centre tap is the row itself) from a hash of the occupied
 * 4 x 4 x 4 BLOCKS of sites: a block's slot (key, 64-bit occupancy mask, payload base) and its rows share cache
 * lines among all the taps that fall into it, where the per-site table costs a line per probed voxel.
 * table: ptv3_subm_block_table_bytes(n) bytes, 16-byte aligned, opaque; build it once per set of sites and query it
 * for any ksize in {1, 3, 5, 7} with the same indices and n.  Every entry of nbr is written (no pre-fill needed). */
size_t ptv3_subm_block_table_bytes(int64_t n);
int ptv3_subm_build_block_table(const int32_t* indices, int64_t n, void* table, size_t bytes, void* stream);
int ptv3_subm_neighbors_blocks(const int32_t* indices, int64_t n, const void* table, size_t bytes, int ksize,
                               int32_t* nbr, void* stream);

/* The executor's form of the table build: ptv3_subm_sites writes indices[i] = (batch[i], grid_coord[i]) as int32
 * (16-byte aligned), optionally the coordinates as (n,3) int64 (grid64, NULL = skip), and zero-fills `table` in the same
 * launch; ptv3_subm_build_block_table_zeroed then builds the table without a fill of its own.  The table is bit for bit
 * the one ptv3_subm_build_block_table builds up to the order of its payload ranges, and the neighbour tables read from
 * it are bit for bit the same. */
int ptv3_subm_sites(const int64_t* batch, const void* grid_coord, int coord_is_i64, int64_t n, int32_t* indices,
                    int64_t* grid64, void* table, size_t bytes, void* stream);
int ptv3_subm_build_block_table_zeroed(const int32_t* indices, int64_t n, void* table, size_t bytes, void* stream);

/* y = epilogue( sum_{d<kvol} sum_{c<cin} w[o][d][c] * x[nbr[i][d]][c] ).
 *   nbr == NULL, kvol == 1  ->  plain torch.nn.Linear: y = x @ w^T            (w: (cout, cin))
 *   nbr != NULL             ->  spconv SubMConv3d, w: (cout, k,k,k, cin) = (cout, kvol, cin)
 * epilogue, in this order, every pointer optional (NULL = skip):
 *   + bias[o];  * bn_scale[o] + bn_shift[o]  (eval BatchNorm1d folded);  act;
 *   y2 = y + res[res_index ? res_index[i] : i][o]   (written to `out2` if given, else into `out`);
 * `out` always receives the pre-residual value when out2 != NULL.
 * row_order (optional, (m) int32): output tile t processes rows row_order[64t..] (locality only).
 * x: (rows_x, cin) dtype - with nbr != NULL, rows_x = m: x is the feature matrix of the m active sites the table was
 * built for (ptv3_subm_neighbors), which lets the kernels address it through a 32-bit buffer descriptor;
 * out/out2/res: (m|rows, cout) dtype; w: dtype; bias/bn_*: fp32.
 * cin % 4 == 0 (fp32) / cin % 8 == 0 (bf16): 16-byte K granularity.
 * workspace (optional): ptv3_gemm_workspace_bytes(...) bytes of split-K slab room; shapes with few
 * rows and a long K (deep-stage convolutions) are then split over K and summed in slab order. */
size_t ptv3_gemm_workspace_bytes(int64_t m, int cin, int cout, int kvol, int dtype);
/* number of K slabs the shape is split into (1 = single pass).  With out == NULL ptv3_gemm leaves the raw fp32
 * slabs [splits][m][cout] in `workspace` for a fused consumer (ptv3_block_head). */
int ptv3_gemm_splits(int64_t m, int cin, int cout, int kvol, int dtype);
int ptv3_gemm(const void* x, const void* w, void* out, int64_t m, int cin, int cout, int kvol,
              const int32_t* nbr, const int32_t* row_order, const float* bias, const float* bn_scale,
              const float* bn_shift, int act, const void* res, const int32_t* res_index, void* out2,
              int dtype, void* workspace, size_t workspace_bytes, void* stream);

/* ---- k^3 stem convolution straight from the block table -------------------------------------------------
 * ptv3_gemm(x, w, out, n, cin, cout, k^3, nbr = the table ptv3_subm_neighbors_blocks(indices, n, table, ksize) gives,
 * row_order, bias, bn_scale, bn_shift, act, no residual, dtype, its workspace) without that (n, k^3) table: a tile of 64
 * sites resolves its neighbour rows from `table` (ptv3_subm_build_block_table[_zeroed] over the same indices and n)
 * into LDS and runs ptv3_gemm's 64-point tile over them.  out is byte-equal to that call in fp32 and bf16, K split
 * included.  ksize 5 (the PTv3 stem) or 3; duplicate coordinates as in the table: the smallest row is the neighbour,
 * every row gets its own output.  x (n, cin), w (cout, ksize^3, cin), out (n, cout) in dtype; indices 16-byte aligned. */
int ptv3_stem_conv_blocks(const void* x, const void* w, void* out, int64_t n, int cin, int cout, int ksize,
                          const int32_t* indices, const void* table, size_t table_bytes, const int32_t* row_order,
                          const float* bias, const float* bn_scale, const float* bn_shift, int act, int dtype,
                          void* stream);

/* ---- narrow 3^3 convolution with the tile's neighbour rows held in LDS --------------------------------
 * ptv3_gemm gathers the rows of x once per tap.  For cin = cout = c in {32, 64} and kvol = 27 the rows a tile of
 * consecutive sites needs can be fetched once instead: ptv3_halo_plan_build cuts the m sites, in row_order, into tiles
 * of T sites and lists per tile its distinct neighbour rows (at most CAP), a 16-bit slot into that list for every
 * (site, tap) (0xFFFF = no neighbour) and the number of distinct rows; ptv3_halo_plan_shape returns (T, CAP).
 * Plan memory, ptv3_halo_plan_bytes(m) bytes, 16-byte aligned, tiles = ceil(m / T):
 *   count: tiles x int32, padded to 16 bytes | rows: tiles x CAP x int32 | slots: tiles x T x 27 x uint16
 * A tile with count > CAP keeps its count and slots, its row list is cut at CAP; ptv3_conv_halo gathers such a tile
 * per tap from global memory inside the same launch.  The plan depends on nbr and row_order alone: build it once per
 * level and share it among the level's convolutions.  Nothing is read back to the host.
 * ptv3_conv_halo: ptv3_gemm(x, w, out, m, c, c, 27, nbr, row_order, ...) with the same epilogue, bitwise the result of
 * its single-pass 64-point tile in fp32 and bf16 (the same matrix-core chain over taps 0..26, zeros for absent
 * neighbours).  nbr and row_order must be the ones the plan was built from.
 * ptv3_conv_halo_policy: 1 where the executor takes ptv3_conv_halo for this shape (PTV3_CONV_HALO = 0 never, 1 the
 * measured policy, 2 every shape the kernel can run), else 0. */
size_t ptv3_halo_plan_bytes(int64_t m);
int ptv3_halo_plan_shape(int* tile_sites, int* cap_rows);
int ptv3_halo_plan_build(const int32_t* nbr, const int32_t* row_order, int64_t m, void* plan, size_t bytes,
                         void* stream);
int ptv3_conv_halo_policy(int64_t m, int cin, int cout, int kvol, int dtype);
int ptv3_conv_halo(const void* x, const void* w, void* out, int64_t m, int c, const int32_t* nbr,
                   const int32_t* row_order, const void* plan, size_t plan_bytes, const float* bias,
                   const float* bn_scale, const float* bn_shift, int act, const void* res, const int32_t* res_index,
                   void* out2, int dtype, void* stream);
/* ptv3_conv_head_halo: ptv3_conv_halo(x, w, t, m, c, nbr, row_order, plan, plan_bytes, conv_bias, ...) followed by
 * ptv3_block_head(t, NULL, 0, NULL, shortcut, g0, b0, g1, b1, wqkv, bqkv, f1, qkv, m, c, eps, ...) as one launch that
 * never writes t: the conv's accumulators are the head's input registers.  f1 and qkv are bitwise those of the two
 * calls, in fp32 and bf16; wqkv is the chain-permuted weight ptv3_block_head takes at c in {32, 64}.  shortcut may be x.
 * ptv3_conv_head_halo_policy: 1 where the executor takes it for a block of m rows (PTV3_CONV_HEAD = 0 never, 1 the
 * measured policy: bf16, c = 64 and m >= a row bound that PTV3_CONV_HEAD_MIN_ROWS overrides, 2 every shape the kernel can
 * run), else 0. */
int ptv3_conv_head_halo_policy(int64_t m, int c, int dtype);
int ptv3_conv_head_halo(const void* x, const void* w, const float* conv_bias, int64_t m, int c, const int32_t* nbr,
                        const int32_t* row_order, const void* plan, size_t plan_bytes, const void* shortcut,
                        const float* g0, const float* b0, const float* g1, const float* b1, const void* wqkv,
                        const float* bqkv, void* f1, void* qkv, float eps, int dtype, void* stream);

/* ---- fused row-local halves of Block.forward (point_transformer_v3m1_base.py:318-338) ----------------
 * ptv3_block_fusable(c, hidden, dtype, m) names the variant the two entry points below will run:
 *   1  c in {32,64} (the large-M levels): one wave carries 16 points through the whole chain in registers
 *      (no LDS, no barrier). bf16: wqkv, w1 (input dim c) and w2 (input dim hidden) must have their input
 *      channels permuted inside every 32-chunk as [0-3,16-19,4-7,20-23,8-11,24-27,12-15,28-31]
 *      (see csrc/block_fused.hip); fp32: natural order.
 *   2  c in {128,256,512}, hidden == 4c: one workgroup per 16 points, its waves split the output channels of
 *      every GEMM, activations hop through LDS; natural weight layout. Every workgroup streams all 12c^2
 *      weights, so the variant is only chosen up to a per-c row limit (default 16384 rows at c=128, off at
 *      256/512; env PTV3_COOP_ROWS_<c>); m = 0 asks for the capability alone.
 *   0  neither (use ptv3_gemm / ptv3_layernorm).
 *   head: x = conv output (or sum of its split-K slabs + conv_bias);
 *         f1 = LN(x; g0,b0) + shortcut;  qkv = LN(f1; g1,b1) @ wqkv^T + bqkv               (:319-324, :188)
 *   tail: f2 = attn @ wproj^T + bproj + f1;  out = f2 + fc2(GELU(fc1(LN(f2; g2,b2))))       (:219, :326-334) */
int ptv3_block_fusable(int c, int hidden, int dtype, int64_t m);
/* One linear layer on whole rows with its LayerNorm neighbours folded in (csrc/block_wide.hip, rows_linear_kernel):
 *   out = act(prologue(x) @ w^T + bias) [+ res],   x (m, c), w (cout, c) natural layout, out / res (m, cout)
 *   g0 == NULL, g1 == NULL : prologue = identity                                   (attn.proj + shortcut, :219)
 *   g0 == NULL, g1 != NULL : prologue = LayerNorm(x; g1, b1)                       (norm2 -> fc1 -> GELU, :330-333)
 *   g0 != NULL             : f1 = LayerNorm(x; g0, b0) + shortcut, stored to `f1`, then LayerNorm(f1; g1, b1)
 *                            (cpe LayerNorm + shortcut -> norm1 -> qkv, :319-324, :188)
 * Every row is read once, the weights stream through LDS (LDS-DMA ring); replaces ptv3_layernorm + ptv3_gemm for
 * c in {128, 256, 512} (fp32: up to 256), cout a multiple of 64 | 32.  ptv3_rows_linear_capable tells whether a shape
 * is served; WHEN to prefer it over the tiled GEMM (row count) is the caller's policy. */
int ptv3_rows_linear_capable(int c, int cout, int dtype, int64_t m);
int ptv3_rows_linear(const void* x, const void* shortcut, const float* g0, const float* b0, const float* g1,
                     const float* b1, const void* w, const float* bias, int act, const void* res, void* f1, void* out,
                     int64_t m, int c, int cout, float eps, int dtype, void* stream);
int ptv3_block_head(const void* x, const float* slab, int splits, const float* conv_bias, const void* shortcut,
                    const float* g0, const float* b0, const float* g1, const float* b1, const void* wqkv,
                    const float* bqkv, void* f1, void* qkv, int64_t m, int c, float eps, int dtype, void* stream);
/* Row-local two-layer MLP, hidden layer in registers (the dense keypoint head, offset_keypoint_ptv3.py:26-31:
 * Linear -> BatchNorm1d(eval) -> ReLU -> Linear):  out = act((x @ w1^T + b1) * s1 + t1) @ w2^T + b2.
 * x (m, cin) dtype, cin in {32, 64}; w1 (hidden, cin) natural; b1 / s1 / t1 (hidden) fp32 (each optional: 0 / 1 / 0);
 * w2 (16 | 32 | 64 rows for cout <= 16 | 32 | 64, hidden) with zero rows beyond cout and, for bf16, its input channels chain-permuted exactly like
 * ptv3_block_tail's w2; b2 (cout) fp32; out (m, cout) fp32 when out_f32 else dtype.  hidden % 64 == 0, cout % 4 == 0,
 * cout <= 64 (ptv3_mlp2_fusable). */
int ptv3_mlp2_fusable(int cin, int hidden, int cout, int dtype);
int ptv3_mlp2(const void* x, const void* w1, const float* b1, const float* s1, const float* t1, int act,
              const void* w2, const float* b2, void* out, int out_f32, int64_t m, int cin, int hidden, int cout,
              int dtype, void* stream);
int ptv3_block_tail(const void* attn, const void* f1, const void* wproj, const float* bproj, const float* g2,
                    const float* b2, const void* w1, const float* bias1, const void* w2, const float* bias2,
                    void* out, int64_t m, int c, int hidden, float eps, int dtype, void* stream);
/* The same tail for few rows (csrc/block_wide.hip, block_tail_sliced_kernel): bf16, c = 128 or 256, hidden = 4 c,
 * weights in natural layout, 64 rows per workgroup.  The hidden layer is cut across `groups` workgroups per row tile
 * (groups divides hidden / 64, at most 16); every group leaves an fp32 partial of `out` in `workspace` ([groups][m][c], 16-byte aligned) and a second
 * launch sums the partials in group order, so the result does not depend on the order the groups finish in.
 * groups = 1 writes `out` directly, bitwise what ptv3_block_tail's streaming kernel writes, and needs no workspace;
 * groups = 0 takes ptv3_block_tail_sliced_policy's count.
 * ptv3_block_tail_sliced_policy: the group count with which the executor takes this tail for a block of m rows, 0
 * where it does not (PTV3_TAIL_SLICED = 0 never, 1 the measured policy: c = 256 from 245 to 4 096 rows, in place
 * of two ptv3_rows_linear and a split-K ptv3_gemm, and c = 128 from 5 590 to 16 384 rows with one group, in place of the
 * cooperative ptv3_block_tail; 2 every m the kernel can run below the rows from which ptv3_block_fusable answers 3;
 * PTV3_TAIL_SLICED_GROUPS names the count). */
int ptv3_block_tail_sliced_policy(int c, int hidden, int dtype, int64_t m);
size_t ptv3_block_tail_sliced_workspace_bytes(int64_t m, int c, int groups);
int ptv3_block_tail_sliced(const void* attn, const void* f1, const void* wproj, const float* bproj, const float* g2,
                           const float* b2, const void* w1, const float* bias1, const void* w2, const float* bias2,
                           void* out, int64_t m, int c, int hidden, float eps, int dtype, int groups, void* workspace,
                           size_t workspace_bytes, void* stream);

/* ---- bottleneck xCPE of PT-v3m1-Plus (pointcept/models/keypoint_ptv3_plus.py:68-94; csrc/cpe_plus.hip) ----------
 * ptv3_rows_linear_ln: cpe[0..2] = SubMConv3d(C, mid, 1, bias=False) -> LayerNorm(mid) -> ReLU (:70-72) in one launch:
 *   out = act(LayerNorm(x @ w^T [+ bias]; gamma, beta, eps)),  x (m, c), w (cout, c), out (m, cout)
 *   c in {16, 32, 64, 128, 256, 512}, cout in {16, 32, 64, 128}.
 * ptv3_subm_conv_ln: cpe[3..5] = SubMConv3d(mid, mid, k, bias=True) -> LayerNorm(mid) -> ReLU (:76-85) in one launch:
 *   out = act(LayerNorm(sum_t w[:, t, :] x[nbr[i][t]] [+ bias]; gamma, beta, eps)),  x / out (m, c), w (c, kvol, c) as
 *   ptv3_gemm takes it, nbr (m, kvol) as ptv3_subm_neighbors writes it, row_order as in ptv3_gemm (locality only);
 *   c in {16, 32, 64, 128}, kvol in {27, 125}.
 * x / w / out in `dtype`, bias / gamma / beta fp32; products accumulate in fp32 and the LayerNorm statistics are taken
 * in fp32 on the unrounded sums, inside one wave in a fixed order (bitwise reproducible).  A table entry outside
 * [0, m) counts as an absent tap.  Any other shape: PTV3_ERR_UNSUPPORTED with ptv3_last_error set, before any launch;
 * the *_capable queries answer the same question without an error. */
int ptv3_rows_linear_ln_capable(int c, int cout, int dtype);
int ptv3_rows_linear_ln(const void* x, const void* w, const float* bias, const float* gamma, const float* beta,
                        void* out, int64_t m, int c, int cout, float eps, int act, int dtype, void* stream);
int ptv3_subm_conv_ln_capable(int c, int kvol, int dtype);
int ptv3_subm_conv_ln(const void* x, const void* w, const int32_t* nbr, const int32_t* row_order, const float* bias,
                      const float* gamma, const float* beta, void* out, int64_t m, int c, int kvol, float eps, int act,
                      int dtype, void* stream);

/* ---- residual-block convolution of SpUNet (pointcept/models/sparse_unet/spconv_unet_v1m1_base.py:72-85, BasicBlock.forward,
 * and :269-273, the decoder's cat(up, skip); csrc/res_conv.hip) ---------------------------------------------------
 * One launch, fp32 (exact-fp32 matrix-core steps):
 *   x[i]       = concat(xa[i] (ca channels), xb[i] (cb channels))          cb = 0, xb = NULL: one source
 *   y[i][o]    = sum_{d<kvol} sum_{c<ca+cb} w[o][d][c] * x[nbr[i][d]][c]   nbr -1 = inactive, as ptv3_gemm
 *   out[i][o]  = act(y * bn_scale[o] + bn_shift[o] + res[i][o])            res optional: the residual BEFORE act
 *   proj[i][o] = (sum_c w_proj[o][c] * x[i][c]) * proj_scale[o] + proj_shift[o]     optional second output, no act
 * w (cout, kvol, ca+cb), w_proj (cout, ca+cb), kvol = 27; nbr (m, 27) and row_order (m) as in ptv3_gemm; xa (m, ca),
 * xb (m, cb), res / out / proj_out (m, cout).  The concatenation is never written and the projection reuses the centre
 * tap's rows of the conv's own operand tile (a non-finite x[nbr[i][d]] of the taps that share a K step with the centre
 * tap reaches proj[i] as NaN).  A table or row_order entry outside [0, m) counts as absent.
 * ca, cb, cout multiples of 4, ca >= 4, ca + cb <= 1024, cout <= 512 (ptv3_res_conv_capable; m only has to be in
 * [1, 2^31)): anything else is refused before any launch, PTV3_ERR_ARG for a malformed call, PTV3_ERR_UNSUPPORTED for
 * a well-formed shape outside the served range.  No allocation, no synchronisation. */
int ptv3_res_conv_capable(int64_t m, int ca, int cb, int cout, int kvol);
/* 16-point row tiles per wave the launch takes for (m, cout): 1 (64-point workgroups) or 2 (128-point workgroups,
 * chosen once they still give every CU two workgroups); 0 for a cout outside [4, 512] or m < 1.  For tests and tools. */
int ptv3_res_conv_row_tiles(int64_t m, int cout);
int ptv3_res_conv(const float* xa, const float* xb, const float* w, const int32_t* nbr, const int32_t* row_order,
                  const float* bn_scale, const float* bn_shift, const float* res, int act, float* out,
                  const float* w_proj, const float* proj_scale, const float* proj_shift, float* proj_out, int64_t m,
                  int ca, int cb, int cout, int kvol, void* stream);

/* ---- normalisation / elementwise -------------------------------------------------------------
 * torch.nn.LayerNorm over the last dim (Block.cpe[2], norm1, norm2; :277-304): y = LN(x)*g+b [+ res];
 * optional second output y2 = LN2(y) * g2 + b2 (fuses `shortcut + cpe` with the following norm1). */
int ptv3_layernorm(const void* x, const float* gamma, const float* beta, const void* res, void* y,
                   const float* gamma2, const float* beta2, void* y2, int64_t m, int c, float eps,
                   int dtype, void* stream);

/* same, with x given as the split-K fp32 slabs a ptv3_gemm(out = NULL) left behind: x = T(sum_z slab[z] + slab_bias)
 * (saves the separate reduce launch and one (m, c) round trip in front of the xCPE LayerNorm, :283) */
int ptv3_layernorm_slabs(const float* slab, int splits, const float* slab_bias, const float* gamma, const float* beta,
                         const void* res, void* y, const float* gamma2, const float* beta2, void* y2, int64_t m, int c,
                         float eps, int dtype, void* stream);

/* y = act(x * scale[c] + shift[c]) : eval BatchNorm1d + GELU of Embedding / SerializedPooling
 * (:508-511, 439-442). In-place allowed. */
int ptv3_affine_act(const void* x, const float* scale, const float* shift, int act, void* y, int64_t m,
                    int c, int dtype, void* stream);

/* dtype conversion helpers (fp32 <-> bf16 storage) */
int ptv3_cast(const void* x, int src_dtype, void* y, int dst_dtype, int64_t count, void* stream);

/* ---- serialized pooling ("grid-pool scatter") ------------------------------------------------
 * replaces torch.unique / torch.sort / cumsum / segment_csr in SerializedPooling.forward
 * (point_transformer_v3m1_base.py:384-428).  Points are visited in serialized order 0, so clusters
 * (equal code0 >> 3*pooling_depth) are contiguous runs of order0.
 * step 1 (segments): cluster[i] (n) int64 = rank of the parent code; seg_start (n+1) int32 run starts
 *         in order0 positions (first *n_out+1 entries valid); n_out written to device AND the
 *         caller reads it back (the one host sync per pooling, as torch.unique has).
 *         batch (n) int64 + pooled_offset (b) int64 (both optional): cumulative scene ends of the
 *         pooled Point (= batch2offset(batch[head]), models/utils/misc.py:32-34); pooled_offset[b-1]
 *         equals n_out.  Each entry is written from its scene's last point: a scene WITHOUT points
 *         keeps what the caller put there (ops.pool_segments pre-fills -1 and forward-fills on the
 *         host; ptv3_forward refuses empty scenes).  workspace: ptv3_pool_workspace_bytes(n). */
size_t ptv3_pool_workspace_bytes(int64_t n);
int ptv3_pool_segments(const int64_t* code0, const int64_t* order0, int64_t n, int shift_bits,
                       const int64_t* batch, int64_t* cluster, int32_t* seg_start, int32_t* n_out,
                       int64_t* pooled_offset, void* workspace, size_t workspace_bytes, void* stream);
/* step 2 (reduce): for pooled row j over members order0[seg_start[j] .. seg_start[j+1]):
 *   feat_out[j]  = act(max_members(feat[.]) * bn_scale + bn_shift)        (n_out, c) dtype
 *   coord_out[j] = mean_members(coord[.])                                  (n_out, 3) fp32
 *   head = first member: grid_out[j] = grid_coord[head] >> pooling_depth (int64), batch_out[j] =
 *   batch[head], code_out[r][j] = code[perm[r]][head] >> 3*pooling_depth for r < k, where perm is the
 *   order shuffle of :408-412 (row_perm_host, k host ints; NULL = identity).
 *   feat == NULL skips the feature half, grid_coord == NULL skips the geometry half (the executor runs the
 *   two halves on different streams). */
int ptv3_pool_reduce(const void* feat, const float* coord, const int64_t* grid_coord,
                     const int64_t* batch, const int64_t* code, int k, const int64_t* order0,
                     const int32_t* seg_start, int64_t n, int64_t n_out, int c, int pooling_depth,
                     const float* bn_scale, const float* bn_shift, int act, const int* row_perm_host,
                     void* feat_out, float* coord_out, int64_t* grid_out, int64_t* batch_out,
                     int64_t* code_out, int dtype, void* stream);

/* ---- whole-model forward ------------------------------------------------------------------------
 * PointTransformerV3.forward (point_transformer_v3m1_base.py:699-714) in eval mode, optionally followed by
 * the dense keypoint-offset head (offset_keypoint_ptv3.py:26-31), as one call: every kernel above is
 * launched back to back from native code.  Used by pointcept.models (PT-v3m1) as its fast path; results
 * are identical to composing the per-op entry points.
 * params: flat table of device pointers in module order -
 *   stem conv w, stem BN scale, shift;
 *   per encoder stage s: [s>0: down.proj w, b, BN scale, shift] then per block the 16 pointers
 *     cpe conv w, b (with the cpe Linear folded in: W'_d = W_lin W_d, b' = W_lin b_conv + b_lin),
 *     cpe LN g, b, norm1 g, b, qkv w, b, proj w, b, norm2 g, b, fc1 w, b, fc2 w, b;
 *   per decoder stage s = S-2..0: up.proj w, b, BN scale, shift, up.proj_skip w, b, BN scale, shift, blocks;
 *   head (if head_out > 0): linear0 w, b, BN scale, shift, linear1 w, b.
 *   matrices in `dtype` (conv weights (cout, kvol, cin) with cin padded to the 16-byte granule),
 *   vectors fp32, BatchNorm folded to (scale, shift). */
typedef struct {
  int32_t dtype, in_channels /* padded */, num_stages, num_orders;
  int32_t enc_depths[8], enc_channels[8], enc_heads[8], enc_patch[8];
  int32_t dec_depths[8], dec_channels[8], dec_heads[8], dec_patch[8];
  int32_t stride[8];
  int32_t enc_mode, enable_flash; /* enable_flash = 0: patch = min(smallest scene, patch) (:173-176) */
  int32_t head_hidden, head_out;  /* head_out = 0: backbone only */
  float mlp_ratio, ln_eps, qk_scale /* 0: (c/heads)^-0.5 */;
} ptv3_model_desc;

typedef struct {
  const void* grid_coord; int32_t coord_is_i64; /* (n,3) */
  const void* feat;                             /* (n, in_channels) dtype */
  const int64_t* batch;                         /* (n), or NULL: derived from offset (misc.py:25-30) */
  const int64_t* offset;                        /* (b) cumulative, device */
  const int64_t* offset_host;                   /* (b) same values on the host, or NULL: read back internally */
  int32_t b; int64_t n;
  int32_t depth;                                /* bit_length(max(grid_coord)+1) (structure.py:73); 0: computed */
  const int32_t* order_ids_host;                /* num_orders curve ids, already in shuffled order */
  const int32_t* pool_perm_host;                /* (num_stages-1, num_orders) row permutations (:408-412) */
  int64_t *code, *order, *inverse;              /* out: (num_orders, n) level-0 serialization */
  void* out_feat;                               /* out: (n, dec_channels[0]) dtype */
  float* out_head;                              /* out: (n, head_out) fp32 (head_out > 0) */
  int64_t* stage_points_host;                   /* out, optional: num_stages point counts */
  int32_t* depth_out;                           /* out, optional: the serialization depth used */
  int64_t* batch_out;                           /* out, optional (batch == NULL): (n) derived batch ids */
  int32_t inputs_resident;                      /* 1: grid_coord / batch / offset were complete in memory before
                                                   this call (not produced on `stream` just now): the geometry
                                                   pipeline may then overlap the previous call's feature tail */
  int32_t overlap_calls;                        /* 1 (needs inputs_resident, parameters unchanged since an earlier
                                                   synchronised call): the feature pipeline runs on one of two
                                                   executor-owned streams instead of `stream`, so the small, latency-
                                                   bound deep levels of call i execute under the chip-filling level-0
                                                   kernels of call i+1.  `stream` only receives a wait on this call's
                                                   completion.  Contract: out_feat / out_head must not be buffers whose
                                                   last readers were enqueued on `stream` after the PREVIOUS call was
                                                   issued (use a ring of >= 3 output buffers, consume call i's outputs
                                                   before issuing call i+2). */
  const void* raw_feat;                         /* overlap mode, optional: (n, raw_feat_channels) features still in   */
  int32_t raw_feat_channels;                    /* their original dtype / width; the executor pads them to            */
  int32_t raw_feat_dtype;                       /* desc->in_channels and casts to desc->dtype on its own stream       */
  int64_t arena_n;                              /* > 0: the workspace was sized by ptv3_forward_workspace_bytes(desc,  */
  int32_t arena_b;                              /* arena_n, arena_b) with arena_n >= n, arena_b >= b: the four arena    */
                                                /* parts then sit at offsets that depend on (arena_n, arena_b) only.   */
                                                /* REQUIRED whenever calls may still be in flight (inputs_resident /    */
                                                /* overlap_calls) and scene sizes vary: with 0 the parts are laid out   */
                                                /* for THIS call's n and would move under the previous call's kernels.  */
  void* executor;                               /* ptv3_executor_create() handle, or NULL = the current device's default */
                                                /* executor.  An executor owns the internal streams / events / call     */
                                                /* parity; calls on one executor are ordered as described above, calls  */
                                                /* on different executors (other models, other devices) are independent. */
} ptv3_forward_io;

/* Executor handles (optional).  create() binds to the CURRENT device; destroy() drains the executor's streams.
 * Every workspace handed to ptv3_forward with inputs_resident / overlap_calls must stay with ONE executor. */
void* ptv3_executor_create(void);
int ptv3_executor_destroy(void* executor);

size_t ptv3_forward_workspace_bytes(const ptv3_model_desc* desc, int64_t n, int b);  /* sized for overlap_calls too */
int ptv3_forward(const ptv3_model_desc* desc, const void* const* params, int num_params,
                 const ptv3_forward_io* io, void* workspace, size_t workspace_bytes, void* stream);

/* ---- training: backward kernels ---------------------------------------------------
 * The reference has no hand-written backward on this path: torch autograd differentiates the forward
 * statements cited at each forward entry point above.  These entry points are what a torch.autograd.Function
 * per layer calls (pointcept-keypointdetection_amd/ptv3_hip/autograd.py).  All reductions over points use
 * fixed row chunks -> fp32 slabs -> ordered sums (deterministic, no atomics).
 *
 * dw (cout, kvol*cin) fp32 = dy^T (m, cout) . gather(x (m, cin) through nbr (m, kvol))   [kvol=1: nbr NULL]
 *   = weight gradient of nn.Linear (point_transformer_v3m1_base.py:188,219,232-244) and of SubMConv3d
 *   (:277-284, 499-506) in the layout of ptv3_gemm's w.  Input gradients reuse ptv3_gemm itself: linear with
 *   w^T; sparse conv with w'[c][t][o] = w[o][kvol-1-t][c] (submanifold neighbour maps are symmetric).
 * dbias (cout) fp32 or NULL: the bias gradient sum_i dy[i][:] from the same pass (the staging of dy sees every
 *   element once; a separate column reduction would read dy again and cost two more launches per layer).
 * m == 0: dw and dbias are zeroed; dy, x and nbr are not read and may be NULL. */
size_t ptv3_gemm_tn_workspace_bytes(int64_t m, int cout, int cin, int kvol);
int ptv3_gemm_tn(const void* dy, const void* x, const int32_t* nbr, float* dw, float* dbias, int64_t m, int cout,
                 int cin, int kvol, int dtype, void* workspace, size_t workspace_bytes, void* stream);
/* column reductions over the m rows of a (and b), out fp32:
 *   mode 0: out[c]       = sum a                          (bias gradients)
 *   mode 1: out[2][c]    = sum a, sum a*a                 (BatchNorm1d batch statistics, :439-441, 508-510)
 *   mode 2: out[2][c]    = sum a, sum a*(b - mu)*rs       (BatchNorm1d backward: a = dy, b = x)
 *   mode 3: out[2][c]    = sum a, sum (a - mu)^2          (centred second pass of the batch variance) */
size_t ptv3_col_reduce_workspace_bytes(int64_t m, int c);
int ptv3_col_reduce(const void* a, const void* b, const float* mu, const float* rs, float mu_scale, int mode, float* out,
                    int64_t m, int c, int dtype, void* workspace, size_t workspace_bytes, void* stream);
/* modes 2 and 3 subtract mu[c] * mu_scale: with mu = the column sums of a first pass and mu_scale = 1 / m the mean never
 * exists as a tensor.
 * The per-channel arithmetic of a BatchNorm1d training step (:439-441, 508-510, the head of offset_keypoint_ptv3.py) in one
 * launch each.  ptv3_bn_finalize: sum / centred_sq (c) = the two col_reduce passes; writes mean, rstd, scale = weight rstd,
 * shift = bias - mean scale and updates the running buffers (NULL: none) with `momentum` and the unbiased variance, as
 * torch.nn.BatchNorm1d does.  ptv3_bn_bwd_coeffs: sums (2, c) = col_reduce mode 2 of the pre-activation gradient; writes
 * the coefficients of ptv3_affine2 (dx = ca dy + cb x + cc). */
int ptv3_bn_finalize(const float* sum, const float* centred_sq, int64_t m, const float* weight, const float* bias,
                     float* running_mean, float* running_var, float momentum, float eps, float* mean, float* rstd,
                     float* scale, float* shift, int c, void* stream);
int ptv3_bn_bwd_coeffs(const float* sums, int64_t m, const float* weight, const float* rstd, const float* mean, float* ca,
                       float* cb, float* cc, int c, void* stream);
/* LayerNorm backward (statistics recomputed from x): dx (m, c) dtype, dgamma_dbeta (2, c) fp32.
 * add (m, c) dtype or NULL: dx = add + (input gradient) - the gradient arriving over the residual connection around the
 * normalised branch (Block.forward, :318-338), folded into the store.  workspace: ptv3_col_reduce_workspace_bytes(m, c). */
int ptv3_layernorm_bwd(const void* x, const void* dy, const void* add, const float* gamma, float eps, void* dx,
                       float* dgamma_dbeta, int64_t m, int c, int dtype, void* workspace,
                       size_t workspace_bytes, void* stream);
/* dx = dy * act'(x * scale[c] + shift[c])  (scale = shift = NULL: act'(x)); act = PTV3_ACT_* */
int ptv3_act_bwd(const void* dy, const void* x, const float* scale, const float* shift, int act, void* dx,
                 int64_t m, int c, int dtype, void* stream);
/* dx = ca[c]*dy + cb[c]*x + cc[c]: BatchNorm1d input gradient with the batch statistics folded into ca/cb/cc */
int ptv3_affine2(const void* dy, const void* x, const float* ca, const float* cb, const float* cc, void* dx,
                 int64_t m, int c, int dtype, void* stream);
/* SerializedPooling segment-max backward (:416-421): the first member holding the maximum gets dy, others 0;
 * SerializedUnpooling gather backward (:480): out[j] = sum of dy over the members of segment j. */
int ptv3_pool_max_bwd(const void* feat, const void* dy, const int64_t* order0, const int32_t* seg_start,
                      int64_t n_out, int c, void* dfeat, int dtype, void* stream);
int ptv3_segment_sum(const void* dy, const int64_t* order0, const int32_t* seg_start, int64_t n_out, int c,
                     void* out, int dtype, void* stream);
/* window attention backward (:196-204 differentiated): qkv (n, 3c), out = forward output (n, c), dout (n, c)
 * -> dqkv (n, 3c).  Softmax statistics are recomputed (nothing saved by the forward). rpe bias unsupported. */
size_t ptv3_window_attn_bwd_workspace_bytes(int64_t n, int64_t n_pad, int c, int heads, int dtype);
int ptv3_window_attn_bwd(const void* qkv, const void* out, const void* dout, const int32_t* win_order,
                         const int32_t* win_inverse, void* dqkv, int64_t n, int64_t n_pad, int c, int heads,
                         int patch, float scale, int dtype, void* workspace, size_t workspace_bytes,
                         void* stream);
/* backward of ptv3_window_attn_varlen_fwd (ragged windows; same workspace size) */
int ptv3_window_attn_varlen_bwd(const void* qkv, const void* out, const void* dout, const int32_t* win_order,
                                const int32_t* win_inverse, const int32_t* cu_seqlens, int num_windows, void* dqkv,
                                int64_t n, int64_t n_pad, int c, int heads, int max_seqlen, float scale, int dtype,
                                void* workspace, size_t workspace_bytes, void* stream);
/* Training pair of the attention: the forward also leaves the log2-domain log-sum-exp of every (padded slot, head) row
 * (lse: n_pad x heads floats), the backward takes it instead of recomputing it in its first pass (a third of that pass's
 * work).  cu_seqlens NULL: uniform windows of `patch` slots, else ragged ones (patch = max_seqlen, sum_len_sq for the flop
 * count).  Same kernels and results as ptv3_window_attn_fwd / _varlen_fwd; dqkv differs from ptv3_window_attn_bwd's only
 * by the summation the two log-sum-exps went through.  workspace: ptv3_window_attn_bwd_workspace_bytes. */
int ptv3_window_attn_train_fwd(const void* qkv, const int32_t* win_order, const int32_t* win_inverse,
                               const int32_t* cu_seqlens, int num_windows, void* out, float* lse, int64_t n,
                               int64_t n_pad, int c, int heads, int patch, float scale, double sum_len_sq, int dtype,
                               void* stream);
int ptv3_window_attn_train_bwd(const void* qkv, const void* out, const void* dout, const float* lse,
                               const int32_t* win_order, const int32_t* win_inverse, const int32_t* cu_seqlens,
                               int num_windows, void* dqkv, int64_t n, int64_t n_pad, int c, int heads, int patch,
                               float scale, int dtype, void* workspace, size_t workspace_bytes, void* stream);
/* Attention dropout in training (reference: nn.Dropout on the attention probabilities,
 * point_transformer_v3m1_base.py:203; flash_attn dropout_p, :211): out_i = sum_j keep_ij softmax(s)_ij v_j / (1 - p).
 * keep_ij is a counter-based hash of (padded query slot, head, key slot in the window) and `seed` (csrc/common.h
 * drop_keep), regenerated by the backward from the same seed - nothing is stored.  The reference's Philox stream is
 * not reproduced: same distribution, different values.  cu_seqlens NULL: uniform windows of `patch` slots, else the
 * ragged layout of ptv3_window_attn_varlen_fwd (patch = max_seqlen).  0 < p_drop < 1.  No rpe bias.
 * The backward takes the forward's out, p_drop and seed; workspace as ptv3_window_attn_bwd_workspace_bytes. */
int ptv3_window_attn_drop_fwd(const void* qkv, const int32_t* win_order, const int32_t* win_inverse,
                              const int32_t* cu_seqlens, int num_windows, void* out, int64_t n, int64_t n_pad, int c,
                              int heads, int patch, float scale, float p_drop, uint32_t seed, int dtype, void* stream);
int ptv3_window_attn_drop_bwd(const void* qkv, const void* out, const void* dout, const int32_t* win_order,
                              const int32_t* win_inverse, const int32_t* cu_seqlens, int num_windows, void* dqkv,
                              int64_t n, int64_t n_pad, int c, int heads, int patch, float scale, float p_drop,
                              uint32_t seed, int dtype, void* workspace, size_t workspace_bytes, void* stream);
/* backward of ptv3_window_attn_rpe_fwd: dqkv as above with the relative-position bias inside the recomputed softmax,
 * plus the gradient of the bias table, dtable (3*(2*pos_bnd+1), heads) fp32 = sum over all (window, query, key) pairs
 * of dS routed to the three (axis, clamped coordinate difference) entries the pair read (RPE.forward,
 * point_transformer_v3m1_base.py:29-48, differentiated).  Per-workgroup partial columns are summed in a fixed order.
 * PTV3_ERR_UNSUPPORTED when 3*(2*pos_bnd+1) > 1024. */
size_t ptv3_window_attn_rpe_bwd_workspace_bytes(int64_t n, int64_t n_pad, int c, int heads, int patch, int pos_bnd,
                                                int dtype);
int ptv3_window_attn_rpe_bwd(const void* qkv, const void* out, const void* dout, const int32_t* win_order,
                             const int32_t* win_inverse, const int32_t* grid_coord, const float* rpe_table,
                             int pos_bnd, void* dqkv, float* dtable, int64_t n, int64_t n_pad, int c, int heads,
                             int patch, float scale, int dtype, void* workspace, size_t workspace_bytes, void* stream);
/* ---- one Block, training, as two native calls -------------------------------------------------------------------
 * Block.forward (point_transformer_v3m1_base.py:318-338, pre-norm, LayerNorm / GELU) and what torch autograd derives
 * from it, each as ONE C call issuing the same kernels as the per-op entry points above would (ptv3_hip/autograd.py
 * BlockFn composes those and is this descriptor's checker):
 *   c = LN0(lin(conv(conv_feat))); f1 = feat + c; f2 = f1 + mask1 * proj(attn(qkv(LN1(f1))));
 *   out = f2 + mask2 * fc2(GELU(fc1(LN2(f2))))
 * All (n, .) tensors in `dtype`, vectors / gradients of parameters fp32.  w_*: (cout, K) as ptv3_gemm's w; wt_*
 * (backward): W^T (cin, cout) of the linears, the mirrored-tap transposed weight (cin, kvol*cout) of the conv.
 * conv_feat NULL: the xCPE conv reads feat (every block but the first decoder block of a stage).  mask1 / mask2 (n) fp32
 * or NULL: uniform draws u; the per-point DropPath factor of a branch is u[i] < keep ? 1 / keep : 0 (timm drop_path with
 * scale_by_keep on the (N, C) matrix).  cu_seqlens NULL: uniform windows of `patch` slots.
 * fwd writes c1 .. out and attn_lse; bwd reads them plus dout and writes dfeat (and dconv_feat), dw_* (cout, K), db_* (cout),
 * dln0/1/2 (2, c) = [dgamma | dbeta] of the three LayerNorms.  workspace: ptv3_block_train_workspace_bytes(). */
typedef struct ptv3_block_train {
  int64_t n, n_pad;
  int32_t c, hidden, heads, patch, kvol, num_windows, dtype, reserved;
  float scale, eps, keep1, keep2;
  double sum_len_sq;
  const int32_t *nbr, *row_order, *win_order, *win_inverse, *cu_seqlens;
  const void *feat, *conv_feat;
  const void *w_conv, *w_lin, *w_qkv, *w_proj, *w_fc1, *w_fc2;
  const void *wt_conv, *wt_lin, *wt_qkv, *wt_proj, *wt_fc1, *wt_fc2;
  const float *b_conv, *b_lin, *b_qkv, *b_proj, *b_fc1, *b_fc2, *g0, *b0, *g1, *b1, *g2, *b2;
  const float *mask1, *mask2;
  void *c1, *c2, *f1, *t3, *qkv, *a, *f2, *t5, *h0, *h, *out;
  const void* dout;
  void *dfeat, *dconv_feat;
  float *dw_conv, *dw_lin, *dw_qkv, *dw_proj, *dw_fc1, *dw_fc2;
  float *db_conv, *db_lin, *db_qkv, *db_proj, *db_fc1, *db_fc2;
  float *dln0, *dln1, *dln2;
  void* workspace;
  size_t workspace_bytes;
  float* attn_lse;   /* (n_pad, heads) fp32: written by fwd, read by bwd (ptv3_window_attn_train_fwd / _bwd) */
} ptv3_block_train;
size_t ptv3_block_train_workspace_bytes(const ptv3_block_train* block, int backward);
int ptv3_block_train_fwd(const ptv3_block_train* block, void* stream);
int ptv3_block_train_bwd(const ptv3_block_train* block, void* stream);

/* fused multi-tensor AdamW (torch.optim.AdamW semantics; pointcept/utils/optimizer.py builds it with one
 * extra "block" parameter group): a device table of ptv3_adamw_entry_bytes()-sized entries, filled on the
 * host by ptv3_adamw_fill_entry; entry i owns blocks [first_block_i, first_block_i + ceil(numel_i / chunk)).
 * fp32 params / grads / moments.  grad_scale multiplies every gradient (1/loss-scale or a clip factor).
 * ptv3_grad_sqnorm: out[0] = sum of squares of all gradients (clip_grad_norm_), partial_ws (total_blocks). */
size_t ptv3_adamw_entry_bytes(void);
int ptv3_adamw_chunk(void);
int ptv3_adamw_fill_entry(void* entry_host, void* param, const void* grad, void* exp_avg, void* exp_avg_sq,
                          int64_t numel, int group, int first_block);
/* optional, after ptv3_adamw_fill_entry: the step also writes the updated parameter into `shadow` (same layout, fp32 or
 * bf16) and, when shadow_t is given, into a (cols, kvol mirrored, rows) transposed copy of the (rows, kvol, cols) weight
 * - W^T of a Linear (kvol 1) / the mirrored-tap weight of a SubMConv3d input gradient - so the training kernels never
 * cast or transpose weights between steps. */
int ptv3_adamw_fill_shadow(void* entry_host, void* shadow, void* shadow_t, int rows, int cols, int kvol,
                           int shadow_dtype);
/* optional, after ptv3_adamw_fill_entry: this tensor has taken `step_lag` steps fewer than the `step` argument of
 * ptv3_adamw_step (torch.optim.AdamW keeps state["step"] per parameter: a parameter that first receives a gradient
 * later, or a resumed checkpoint, engines/hooks/misc.py:269); its bias corrections use step - step_lag. */
int ptv3_adamw_fill_step_lag(void* entry_host, int64_t step_lag);
/* the transposed shadows are written by a second pass of 64 x 64 tiles: entry i owns tiles [first_tile_i, first_tile_i +
 * ptv3_adamw_shadow_tiles(rows, cols, kvol)) when it has a shadow_t and none otherwise (first_tile_i = the running sum,
 * set on EVERY entry); total_tiles / shadow_dtype of ptv3_adamw_step describe that pass (0 tiles: no shadow_t anywhere). */
int ptv3_adamw_shadow_tiles(int rows, int cols, int kvol);
int ptv3_adamw_fill_first_tile(void* entry_host, int first_tile);
/* grads_host (ntensors host array of device pointers) or NULL: this step's gradient of every table entry, overriding the
 * address stored in the table.  torch's autograd leaves a new gradient tensor on each parameter after
 * zero_grad(set_to_none=True) (no zero fill, no accumulate-add per parameter); the addresses travel as kernel arguments,
 * 256 tensors per launch, so the table is neither rebuilt nor re-uploaded.  first_block_host (ntensors): the
 * first_block given to ptv3_adamw_fill_entry for every entry (required with grads_host).  A gradient address may be
 * NULL only for an entry of zero elements (it owns no block); for any other entry the call is refused. */
int ptv3_adamw_step(const void* table_dev, int ntensors, int total_blocks, const float* lr_host,
                    const float* wd_host, int ngroups, float beta1, float beta2, float eps, int64_t step,
                    float grad_scale, const int32_t* first_block_host, const void* const* grads_host, int total_tiles,
                    int shadow_dtype, void* stream);
int ptv3_grad_sqnorm(const void* table_dev, int ntensors, int total_blocks, float* partial_ws, float* out,
                     const int32_t* first_block_host, const void* const* grads_host, void* stream);

/* ---- GridSample (the step before the model) -----------------------------------------------------------
 * Front half of pointcept/datasets/transform.py:848-860 for one cloud: grid_coord = floor(coord / grid_size)
 * evaluated in float64 as numpy does (float32 coord / float64 grid size), minus its per-axis minimum; key = the
 * reference's voxel hash of the shifted coordinate (:926-964).  coord (n,3) fp32; grid_coord (n,3) int64 out;
 * min_max (6) int64 out = [min xyz, max xyz] of the unshifted voxel coordinate; key (n) uint64 out.
 * The rest of GridSample composes existing entry points: ptv3_argsort_i64(key, end_bit 64) = np.argsort,
 * ptv3_pool_segments(key, order, shift 0) = np.unique(return_inverse, return_counts). */
#define PTV3_HASH_FNV 0
#define PTV3_HASH_RAVEL 1
int ptv3_grid_hash(const float* coord, int64_t n, double grid_size, int hash_type, int64_t* grid_coord,
                   int64_t* min_max, uint64_t* key, void* stream);

/* ---- keypoint aggregation (the step after the model) -------------------------------------------------
 * One launch for the per-sample x per-keypoint python loops of engines/hooks/offset_keypoint_evaluator.py:46-84
 * and tools/infer_offset.py:555-597.  coord (N,3) fp32; pred (N, nkp, 4) fp32 = [offset xyz, score] (model output
 * or target); offset (nscenes) cumulative int64; scale (nscenes) / centroid (nscenes,3) fp32 or NULL (1 / 0).
 * point(i) = coord[i]*scale + centroid + pred[i][k][0:3]*scale  (each step rounded as the torch statements).
 *   PTV3_KP_ARGMAX    kp = point(first arg max of the score)                    aux = that index within the scene
 *   PTV3_KP_WEIGHTED  kp = sum w point / sum w over score > thresh, arg max if none (infer_offset "weighted")
 *                                                                               aux = # points over thresh
 *   PTV3_KP_GT_MEAN   kp = mean of point(i) over score > 0 (evaluator :49-53)   aux = # such points, NaN if 0
 *   PTV3_KP_GT_FIRST  kp = point(first i with score > 0.5) (infer_offset :592-596)  aux = that index or -1 (NaN)
 * kp_out (nscenes, nkp, 3) fp32, aux_out (nscenes, nkp) int32. */
#define PTV3_KP_ARGMAX 0
#define PTV3_KP_WEIGHTED 1
#define PTV3_KP_GT_MEAN 2
#define PTV3_KP_GT_FIRST 3
int ptv3_keypoint_aggregate(const float* coord, const float* pred, const int64_t* offset, int nscenes, int nkp,
                            const float* scale, const float* centroid, int mode, float thresh, float* kp_out,
                            int32_t* aux_out, void* stream);

/* ---- global-regression keypoint heads (KeypointPTv3 / KeypointSwin3D) --------------------------------------
 * ptv3_scene_mean: out (b, c) fp32 = per-scene column mean of feat (n, c) fp32 / bf16, scenes given by the cumulative
 *   int64 offset (b) - torch_scatter.scatter_mean(feat, point.batch, dim=0) of pointcept/models/keypoint_ptv3.py:44 and
 *   the per-scene feat[start:end].mean(dim=0) loop of pointcept/models/keypoint_swin3d.py:109-117.  An empty scene
 *   gives a zero row (scatter_mean).  Accumulates in fp32; deterministic (fixed row chunks that never straddle a scene
 *   -> fp32 slabs -> per-scene ordered sum, two launches, no atomics); the grid is sized from n and b only (no read of
 *   offset on the host).  c a multiple of 8 in [8, 1024]; feat, out and workspace 16-byte aligned.
 * ptv3_scene_mean_head: the same pooling, then the regression head of keypoint_ptv3.py:24-32 / keypoint_swin3d.py:
 *   30-38 in eval mode on the pooled rows, fp32: out (b, out_dim) = W3 relu(W2 relu((W1 g + b1) s1 + t1) + b2) + b3,
 *   s1 / t1 = the folded BatchNorm1d, Dropout the identity.  Weights TRANSPOSED: w1t (c, hidden), w2t (hidden, hidden),
 *   w3t (hidden, out_dim); hidden, out_dim in [1, 1024].  Two launches.
 * ptv3_scene_mean_bwd: dfeat (n, c) in dtype: dfeat[i] = dg[scene(i)] / n_scene(i) (the backward of the mean; rows
 *   past offset[b-1] get 0).  workspace: ptv3_scene_mean_workspace_bytes(n, c, b). */
size_t ptv3_scene_mean_workspace_bytes(int64_t n, int c, int b);
int ptv3_scene_mean(const void* feat, const int64_t* offset, int64_t n, int c, int b, int dtype, float* out,
                    void* workspace, size_t workspace_bytes, void* stream);
int ptv3_scene_mean_head(const void* feat, const int64_t* offset, int64_t n, int c, int b, int dtype, const float* w1t,
                         const float* b1, const float* s1, const float* t1, int hidden, const float* w2t,
                         const float* b2, const float* w3t, const float* b3, int out_dim, float* out, void* workspace,
                         size_t workspace_bytes, void* stream);
int ptv3_scene_mean_bwd(const float* dg, const int64_t* offset, int64_t n, int c, int b, void* dfeat, int dtype,
                        void* stream);

/* ---- classifier / regressor head (DefaultClassifier, PigBodyRegressor; csrc/cls_head.hip) ---------------------
 * The part of pointcept/models/default.py:289-338 after the backbone: torch_scatter.segment_csr(feat, offset, "mean")
 * (:322-326), cls_head = Linear(c, h1) -> BatchNorm1d -> ReLU -> Dropout -> Linear(h1, h2) -> BatchNorm1d -> ReLU ->
 * Dropout -> Linear(h2, out) (:303-313, :330), and - when `target` (b * out) is given - RegressionL1Loss
 * (pointcept/models/losses/weight_regression_loss.py:30-38) with the column errors PigBodyRegressor logs
 * (pointcept/models/pig_regressor.py:36-55): stats (1 + out) = { loss_weight * mean |logit - target|,
 * metric_scale * mean over rows |logit - target| per column }.  Everything is fp32; no atomics, sums in a fixed order
 * (two runs are bitwise equal).  Rows are walked in tiles of PTV3_CLS_HEAD_ROW_TILE inside one workgroup, any b.
 * Limits: c a multiple of 8 in [8, 1024]; h1, h2, out each in [1, 512] (ptv3_cls_head_capable answers without an
 * error); outside them PTV3_ERR_UNSUPPORTED with ptv3_last_error set, before any launch.
 * ptv3_cls_head_eval: feat (n, c) fp32 / bf16 -> logits (b, out).  Two launches: the pooling partials of
 *   ptv3_scene_mean, then one workgroup that sums every scene's slabs in ptv3_scene_mean's order (an empty scene gives
 *   a zero row) and runs the head with the BatchNorms folded into (s, t) and Dropout the identity.  Weights TRANSPOSED:
 *   w1t (c, h1), w2t (h1, h2), w3t (h2, out).  workspace: ptv3_scene_mean_workspace_bytes(n, c, b).
 * ptv3_cls_head_train_fwd: g (b, c) pooled rows -> logits (+ stats), one launch, b >= 2.  nn.Linear's own (out, in)
 *   weights.  BatchNorm with batch statistics (two-pass variance); running_mean / running_var are updated in place
 *   (momentum, unbiased variance; num_batches_tracked is the caller's).  mask1 (b, h1), mask2 (b, h2): the Dropout
 *   keep-masks (0 / 1), applied as mask * inv_keep.  save: ptv3_cls_head_save_floats(b, h1, h2, out) floats, the tape.
 * ptv3_cls_head_train_bwd: two launches.  dlogits (b, out) given, or formed as dloss[0] * loss_weight *
 *   sign(logit - target) / (b * out) with sign(0) = 0 from the tape (dloss: a DEVICE scalar); exactly one of the two.
 *   The dloss form needs the tape of a forward that was given `target`: a forward without one tapes zero signs, and
 *   every gradient then comes out as zero.
 *   Writes dg (b, c) and the ten parameter gradients; dz: scratch of b * (h1 + h2 + out) floats. */
#define PTV3_CLS_HEAD_ROW_TILE 8
typedef struct ptv3_cls_head_params {
  const float *w1, *b1, *bn1_weight, *bn1_bias;
  float *bn1_running_mean, *bn1_running_var;
  const float *w2, *b2, *bn2_weight, *bn2_bias;
  float *bn2_running_mean, *bn2_running_var;
  const float *w3, *b3;
  float bn1_momentum, bn1_eps, bn2_momentum, bn2_eps;
} ptv3_cls_head_params;
typedef struct ptv3_cls_head_grads {
  float *dw1, *db1, *dbn1_weight, *dbn1_bias, *dw2, *db2, *dbn2_weight, *dbn2_bias, *dw3, *db3;
} ptv3_cls_head_grads;
int ptv3_cls_head_capable(int c, int h1, int h2, int out);
int ptv3_cls_head_eval(const void* feat, const int64_t* offset, int64_t n, int c, int b, int dtype, const float* w1t,
                       const float* b1, const float* s1, const float* t1, int h1, const float* w2t, const float* b2,
                       const float* s2, const float* t2, int h2, const float* w3t, const float* b3, int out,
                       const float* target, float loss_weight, float metric_scale, float* logits, float* stats,
                       void* workspace, size_t workspace_bytes, void* stream);
size_t ptv3_cls_head_save_floats(int b, int h1, int h2, int out);
int ptv3_cls_head_train_fwd(const float* g, int b, int c, int h1, int h2, int out, const ptv3_cls_head_params* params,
                            const float* mask1, const float* mask2, float inv_keep, const float* target,
                            float loss_weight, float metric_scale, float* save, float* logits, float* stats,
                            void* stream);
int ptv3_cls_head_train_bwd(const float* g, int b, int c, int h1, int h2, int out, const ptv3_cls_head_params* params,
                            const float* dlogits, const float* dloss, float loss_weight, float inv_keep, float* save,
                            float* dz, float* dg, const ptv3_cls_head_grads* grads, void* stream);

/* ---- voting keypoint head (KeypointSwin3DVote) ---------------------------------------------------------------
 * ptv3_scene_median: out (b, c) fp32, out[s, j] = the LOWER median over the rows i of scene s of x[i, j]
 *   (+ coord[i, j % 3] when coord (n, 3) is given: one fp32 add inside the kernel, so the (n, K, 3) predicted positions
 *   of pointcept/models/keypoint_swin3d_plus.py:84 never exist) - the per-scene boolean-mask gather plus
 *   sample_votes.median(dim=0).values loop of keypoint_swin3d_plus.py:166-189, without its host synchronisations.
 *   torch.median semantics: rank (rows - 1) / 2 of the ascending order; a NaN in a column gives NaN for that (scene,
 *   column) only; an empty scene gives zeros (:181-183).  The result is one of the inputs, bit for bit: an exact
 *   radix select (four 8-bit passes over an order-preserving key; integer histograms merged with integer atomics, every
 *   hand-off between workgroups a kernel boundary), bitwise reproducible.  x (n, c) fp32 row-major, 1 <= c <= 32, c a
 *   multiple of 3 with coord; offset (b) cumulative int64, clamped into [0, n]; n < 2^31.  workspace:
 *   ptv3_scene_median_workspace_bytes(c, b), 16-byte aligned.  One memset + five launches.
 * ptv3_vote_loss: the training loss and curves of keypoint_swin3d_plus.py:86-164 in two launches.  votes (n, 3k) fp32
 *   are the head's raw offsets; mask[i, j] = |coord_i - target| < radius; loss = sum over the mask of the xyz mean of
 *   smooth-L1(beta = 1) of (coord + votes) - target, / max(mask count, 1).  target: (b * k, 3) indexed by the point's
 *   scene, or with target_per_point (n * k, 3).  scale (optional): (b), or with scale_per_point (n).
 *   out (2 + k) fp32 = loss, train/masked_dist_err, train/kp{j}_dist_err (masked means of the point-to-target distance
 *   times scale, 0 where the count is 0); count (1 + k) int32 = mask total, per keypoint.  Fixed row chunks -> slabs ->
 *   one finishing workgroup (float64 sums, integer counts): no atomics, bitwise reproducible.  1 <= k <= 32.
 *   workspace: ptv3_vote_loss_workspace_bytes(n, k, b), 16-byte aligned.
 * ptv3_vote_loss_bwd: autograd of that loss (:111-117): dvotes (n, 3k) = dloss[0] * mask * clamp((coord + votes) -
 *   target, -1, 1) / (3 * max(count[0], 1)), the mask recomputed; dloss and count stay on the device.  One launch. */
size_t ptv3_scene_median_workspace_bytes(int c, int b);
int ptv3_scene_median(const float* x, const float* coord, const int64_t* offset, int64_t n, int c, int b, float* out,
                      void* workspace, size_t workspace_bytes, void* stream);
size_t ptv3_vote_loss_workspace_bytes(int64_t n, int k, int b);
int ptv3_vote_loss(const float* votes, const float* coord, const float* target, int target_per_point,
                   const int64_t* offset, const float* scale, int scale_per_point, int64_t n, int k, int b, float radius,
                   float* out, int32_t* count, void* workspace, size_t workspace_bytes, void* stream);
int ptv3_vote_loss_bwd(const float* dloss, const float* votes, const float* coord, const float* target,
                       int target_per_point, const int64_t* offset, const int32_t* count, int64_t n, int k, int b,
                       float radius, float* dvotes, void* stream);

/* ---- measurement ---------------------------------------------------------------------------------
 * While enabled, the GEMM / fused-block / attention entry points (forward and backward) bracket their launches with
 * HIP events on the launch stream.  collect() synchronises the device and returns, per kernel family (0 linear,
 * 1 subm_conv, 2 window_attn, 3 backward: arrays of FOUR entries): summed device milliseconds, algorithmic flops
 * (sparse conv: 2*cin*cout per ACTIVE neighbour), algorithmic bytes and launch count since enable / the last collect. */
int ptv3_profile_enable(int on);
int ptv3_profile_collect(double* ms, double* flops, double* bytes, int64_t* launches);
/* Flops of the NEXT bracketed launch, for kernels whose work is decided by device data the entry point does not read
 * back (ptv3_swin_attn_fwd: the pair count sum_w len_w^2 lives in w_start); ignored while profiling is off. */
int ptv3_profile_hint_flops(double flops);
/* the same records by KERNEL (one launch per bracket): arrays of ptv3_profile_kernel_count() entries, entry i is the
 * kernel ptv3_profile_kernel_name(i) (gemm_kernel 64 / 32 channel tiles and gemm_big_kernel each split into their
 * dense and gathered = sparse-conv launches, the fused block halves, mlp2, the two window-attention kernels).  Does not
 * reset the records: call it BEFORE ptv3_profile_collect. */
int ptv3_profile_kernel_count(void);
const char* ptv3_profile_kernel_name(int kernel);
int ptv3_profile_collect_kernels(double* ms, double* flops, double* bytes, int64_t* launches);

/* ---- Swin3D window partition + cRSE window attention (row A19; PARITY UNPINNED) -----------------------------
 * The reference computes these through MinkowskiEngine and microsoft/Swin3D, neither of which is in its tree
 * (SURVEY.md section 8c); oracle/swin3d.py restates them from pointcept/models/swin3d/swin3d_layers.py and the
 * Swin3D paper and is the only checker these two entry points have.
 *
 * ptv3_swin_window_keys replaces the MinkowskiMaxPooling + coordinate_manager.kernel_map part of
 * BasicLayer.get_map_pair / get_window_mapping (swin3d_layers.py:715-795) and get_shifted_sp (:826-840):
 * coords (n,4) int32 [batch, x, y, z] at tensor stride `stride`; voxel = floor(c / stride) + shift; window =
 * floor(voxel / window_size) per axis; key = (batch, window xyz) << 9 | w_w_id with w_w_id = (lx*ws + ly)*ws + lz
 * (:781-788).  ptv3_argsort_i64(key, end_bit 64) is then the reference's sort by in_map (:752), and
 * ptv3_pool_segments(key, order, shift 9) yields the windows' token ranges (nempty_num, :777-778).
 * *bad is set non-zero when a batch index (0..4095) or window coordinate (-4096..4095) does not fit the key. */
int ptv3_swin_window_keys(const int32_t* coords, int64_t n, int stride, int window_size, int shift, int64_t* key,
                          int32_t* bad, void* stream);
/* replaces SelfAttnAIOFunction.apply(..., PosEmb.SEPARATE, TableDims.D0, IndexMode.INDIRECT, ...) at
 * swin3d_layers.py:556-569 (forward; ptv3_swin_attn_bwd below is its backward).  q, k, v, out: (n, heads, head_dim) in ORIGINAL voxel order, q already
 * scaled (:499); {q,k,v}_table: the concatenated fp32 tables of :503-528, table_offsets_host[c] elements per signal
 * axis c (the reference's `table_offsets`, :441/:452/:464), num_axes = 3, 6 or 9; n2n (n) int64: sorted position ->
 * original row (n2n_indices); w_start (num_windows + 1) int32: token range of each window in sorted order
 * (w2n_indices plus the total); n_crse (n, num_axes) fp32 in sorted order (:505-530); max_tokens >= the largest
 * window (window_size^3 always is).  head_dim 8, 16 or 32.
 *   e_ij = q_i.k_j + sum_c (q_i.T_K[c][idx] + k_j.T_Q[c][idx]),  out_i = sum_j softmax_j(e_ij) (v_j + sum_c T_V[c][idx]),
 *   idx = clamp(floor(s_i[c] - s_j[c] + rows_c / 2), 0, rows_c - 1)   in fp32. */
int ptv3_swin_attn_fwd(const void* q, const void* k, const void* v, const float* q_table, const float* k_table,
                       const float* v_table, const int32_t* table_offsets_host, int num_axes, const int64_t* n2n,
                       const int32_t* w_start, int num_windows, const float* n_crse, void* out, int64_t n, int heads,
                       int head_dim, int max_tokens, int dtype, void* stream);

/* backward of ptv3_swin_attn_fwd (the reference: SelfAttnAIOFunction.backward of the absent microsoft/Swin3D; checked
 * against torch autograd over the restated forward: parity unpinned).  dout (n, heads, head_dim) in dtype; writes dq, dk, dv
 * (same shape / dtype) and the fp32 gradients of the three concatenated tables (sum(table_offsets) elements each; zeroed
 * here, then accumulated with atomics: their last bits depend on the order of additions). */
int ptv3_swin_attn_bwd(const void* q, const void* k, const void* v, const void* dout, const float* q_table,
                       const float* k_table, const float* v_table, const int32_t* table_offsets_host, int num_axes,
                       const int64_t* n2n, const int32_t* w_start, int num_windows, const float* n_crse, void* dq,
                       void* dk, void* dv, float* dq_table, float* dk_table, float* dv_table, int64_t n, int heads,
                       int head_dim, int max_tokens, int dtype, void* stream);

/* ---- pointops (libs/pointops) ------------------------------------------------------------------
 * Same argument meaning as the reference's extern "C" launchers
 * (libs/pointops/src/knn_query/knn_query_cuda_kernel.h:9-17, grouping/grouping_cuda_kernel.h,
 * interpolation/interpolation_cuda_kernel.h) plus the stream. */
int ptv3_knn_query(int m, int nsample, const float* xyz, const float* new_xyz, const int* offset,
                   const int* new_offset, int b, int* idx, float* dist2, void* stream);
/* k nearest by a walk over the occupied cells of a uniform grid (cells of edge `cell`, the unit of xyz) instead of a
 * scan of the scene: the k smallest by (distance, candidate index), each row ascending in that order.  Against
 * ptv3_knn_query (= the reference's scan) every row holds the same distances and the same neighbours strictly closer than
 * its k-th distance; which of several candidates AT the k-th distance is kept, and the order inside a group of equal
 * distances, are by-products of the reference's heap and differ (lowest indices here).  nsample = 1: identical.
 * qcell (m,4) int32: [scene, cx, cy, cz] of every query, cx = floor(x / cell) - min over the scene set, 0..65535;
 * table / slots: ptv3_subm_build_table over the DISTINCT candidate cells (ncell,4); order (n) int64 + seg_start
 * (ncell+1) int32: the candidates of cell c are order[seg_start[c] .. seg_start[c+1]) (ptv3_argsort_i64 +
 * ptv3_pool_segments of the candidates' cell keys); offset (b) int32: the candidates' cumulative scene ends.  A query
 * whose k-th neighbour is not settled within 8 shells (sparse surroundings, or a scene with fewer than nsample
 * candidates, which pads with idx -1, dist2 1e10 as ptv3_knn_query does) is answered by a scan of its scene. */
int ptv3_knn_query_cells(int m, int nsample, const float* xyz, const float* new_xyz, const int32_t* qcell,
                         const void* table, int64_t slots, const int64_t* order, const int32_t* seg_start,
                         const int* offset, float cell, int* idx, float* dist2, void* stream);
int ptv3_grouping_forward(int m, int nsample, int c, const float* input, const int* idx, float* output,
                          void* stream);
int ptv3_grouping_backward(int m, int nsample, int c, const float* grad_output, const int* idx,
                           float* grad_input, void* stream);
int ptv3_interpolation_forward(int n, int c, int k, const float* input, const int* idx,
                               const float* weight, float* output, void* stream);
int ptv3_interpolation_backward(int n, int c, int k, const float* grad_output, const int* idx,
                                const float* weight, float* grad_input, void* stream);
/* Farthest point sampling, replacing libs/pointops/src/sampling/sampling_cuda_kernel.cu:15-129 (same arguments as its
 * launcher, plus the stream).  xyz (n,3) fp32; offset / new_offset (b) int32 cumulative ends of the scenes and of their
 * samples; idx (new_offset[b-1]) int32 receives GLOBAL row indices.  Every scene starts at its first point and then
 * repeatedly takes the point whose running minimum squared distance (dx*dx + dy*dy + dz*dz in fp32) to the chosen set is
 * largest.  tmp (n) fp32 is in/out: read as the initial running distances (non-negative; the caller fills it with
 * 1e10), it holds the final ones on return.  One workgroup per scene; n_max (the largest scene) only selects where a
 * scene's state lives (registers up to 16384 points, then 8192 more in LDS, then global memory).  Bitwise reproducible.
 * Two deliberate differences from the reference:
 *   - ties go to the LOWEST index (the reference's tie order depends on its block size), so a scene of identical
 *     points returns its first index repeated;
 *   - a scene asked for zero samples writes nothing (the reference writes idx[start_m] regardless, which lands in the
 *     next scene's slot or past the end). */
int ptv3_farthest_point_sampling(int b, int n_max, const float* xyz, const int* offset, const int* new_offset,
                                 float* tmp, int* idx, void* stream);

/* ---- Point Transformer V1 vector attention, eval forward ------------------------------------------
 * PointTransformerLayer.forward after its three input projections (pointcept/models/point_transformer/
 * point_transformer_seg.py:90-120) in one launch.  x_q / x_k / x_v (n,c) fp32, xyz (n,3) fp32, idx (n,ns) int32 rows of
 * the point's neighbours (-1, or anything outside [0,n), = missing: zero feature rows and a zero offset, as
 * pointops.grouping gives them), out (n,c) fp32.  With j = idx[i,s], cs = c/8 and every BatchNorm folded to a per-channel
 * (scale s, shift t) that also carries the bias of the Linear in front of it:
 *   h   = relu(s_p * (w_p1 (xyz[j] - xyz[i])) + t_p)                     w_p1 (3,3), s_p / t_p (3)
 *   p_r = w_p2 h + b_p2                                                  w_p2 (c,3), b_p2 (c)
 *   a   = relu(s_c * (x_k[j] - x_q[i] + p_r) + t_c)                      s_c / t_c (c)
 *   w   = w_w2 relu(s_w * (w_w1 a) + t_w) + b_w2                         w_w1 (cs,c), s_w / t_w (cs), w_w2 (cs,cs), b_w2 (cs)
 *   w   = softmax over the ns neighbours, per channel of w
 *   out[i, g*cs + t] = sum_s (x_v[j, g*cs + t] + p_r[g*cs + t]) * w[s, t]   for the 8 share groups g
 * c: a multiple of 8 in [8,512]; ns in [1,32]; anything else is refused with PTV3_ERR_ARG before any launch.  fp32
 * arithmetic and accumulation, no atomics: bitwise reproducible. */
int ptv3_vector_attn_fwd(const float* x_q, const float* x_k, const float* x_v, const float* xyz, const int32_t* idx,
                         int64_t n, int c, int ns, const float* w_p1, const float* s_p, const float* t_p,
                         const float* w_p2, const float* b_p2, const float* s_c, const float* t_c, const float* w_w1,
                         const float* s_w, const float* t_w, const float* w_w2, const float* b_w2, float* out,
                         void* stream);

/* ---- OA-CNNs: kernel-2 / stride-2 sparse convolution pair (fp32) -----------------------------------
 * spconv.SparseConv3d(kernel_size=2, stride=2) of DonwBlock.down and spconv.SparseInverseConv3d of UpBlock.up
 * (pointcept/models/oacnns/oacnns_v1m1_base.py:130-141, 184-194; parity with the spconv wheel unpinned).  A fine site
 * (b, x, y, z) has ONE parent (b, x>>1, y>>1, z>>1), reached through tap (x&1)*4 + (y&1)*2 + (z&1); a site whose
 * parent lies outside the coarse shape (sx, sy, sz) has none.
 * plan, step 1: key[i] = ((b*sx + px)*sy + py)*sz + pz, or none_key (> every parent key, so it sorts last) for a
 *   site without a parent; tap[i] (n) int32.  The caller then sorts the keys (ptv3_argsort_i64) and ranks them
 *   (ptv3_pool_segments, shift 0).
 * plan, step 2: from rank / order / seg_start / n_out of those two calls: parent (n) int32 (-1 = none), child
 *   (>= coarse rows, 8) int32 pre-filled with -1 by the caller, coarse (>= coarse rows, 4) int32 sites in (b, x, y, z)
 *   order, up_key (n) int64 = tap, or 8 without a parent (sorted by the caller into up_rows), counts (10) int32
 *   pre-zeroed: [0] coarse rows, [1 + t] sites of tap t, [9] sites without a parent - the ONE host read of a level. */
int ptv3_down2_keys(const int32_t* indices, int64_t n, int sx, int sy, int sz, int64_t none_key, int64_t* key,
                    int32_t* tap, void* stream);
int ptv3_down2_children(const int32_t* indices, const int64_t* key, const int32_t* tap, const int64_t* rank,
                        const int64_t* order, const int32_t* seg_start, const int32_t* n_out, int64_t n,
                        int64_t none_key, int32_t* parent, int32_t* child, int32_t* coarse, int64_t* up_key,
                        int32_t* counts, void* stream);
/* down (:130-141): out[j] = epi(sum_t w[:, t, :] x[child[j][t]]), x (n_in, cin), w (cout, 8, cin), out (m_out, cout);
 * up (:184-194):   out[i] = epi(w[:, tap(i), :] y[parent[i]]), y (m_in, cin), out (n, cout); rows without a parent get
 *   epi(0).  up_rows (n) int32: the rows stably sorted by up_key; tap_start_host: 10 host ints, rows
 *   [tap_start[t], tap_start[t+1]) of up_rows use tap t (t = 8: no parent) - a row costs one tap of multiply work.
 * epi = * bn_scale + bn_shift (optional, together), then act (PTV3_ACT_NONE | PTV3_ACT_RELU).  cin % 4 == 0. */
int ptv3_down2_conv(const float* x, const float* w, const int32_t* child, int64_t n_in, int64_t m_out, int cin, int cout,
                    const float* bn_scale, const float* bn_shift, int act, float* out, void* stream);
int ptv3_up2_conv(const float* y, const float* w, const int32_t* parent, const int32_t* up_rows,
                  const int32_t* tap_start_host, int64_t n, int64_t m_in, int cin, int cout, const float* bn_scale,
                  const float* bn_shift, int act, float* out, void* stream);

/* ---- OA-CNNs: adaptive aggregator of BasicBlock.forward (oacnns_v1m1_base.py:87-110, fp32) -------------
 * Partition (DonwBlock.forward :158-164, torch_geometric voxel_grid + torch.unique): key[i] packs
 * (b, (x - min_x) / g, (y - min_y) / g, (z - min_z) / g) with min_xyz (3) int32 ON THE DEVICE (the minimum over all
 * rows of the batch) and 1 <= g <= 128; ptv3_argsort_i64 + ptv3_pool_segments turn it into order / seg_start /
 * cluster ids, and the cluster count stays on the device (n_clusters): every kernel below is launched for m rows.
 *   center (:92):       out[i] = x[i] - mean over i's cluster of x                          x (m, C) row stride ldx
 *   softmax_sum (:94-97): agg[k] = sum_{i in k} v[i] e[i] / (sum_{i in k} e[i] + 1e-6), e = exp(p - *global_max)
 *                       p, v (m, C) with row strides ldp, ldv; agg (>= clusters, C)
 *   mix (:99-102):      out[i, out_col : out_col + C] = sum_l softmax(logits[i, :L])[l] * agg_l[cluster_l[i]], L <= 4
 *                       agg_host / cluster_host: L host arrays of device pointers; head (optional, (m, C) stride ldh)
 *                       is copied to out[i, 0:C] (the left half of the `fuse` input, :103-104); out row stride ldo
 * C a multiple of 4 in [4, 512]; fp32 accumulation in a fixed order, no atomics: bitwise reproducible; clusters of 1
 * to m rows.  Anything else is refused with PTV3_ERR_ARG before a launch. */
int ptv3_cluster_keys(const int32_t* indices, int64_t m, const int32_t* min_xyz, int g, int64_t* key, void* stream);
int ptv3_cluster_center(const float* x, int64_t ldx, const int64_t* order, const int32_t* seg_start,
                        const int32_t* n_clusters, int64_t m, int c, float* out, void* stream);
int ptv3_cluster_softmax_sum(const float* p, int64_t ldp, const float* v, int64_t ldv, const float* global_max,
                             const int64_t* order, const int32_t* seg_start, const int32_t* n_clusters, int64_t m,
                             int c, float* agg, void* stream);
int ptv3_cluster_mix(const float* logits, int64_t ldl, const float* const* agg_host, const int64_t* const* cluster_host,
                     int levels, const float* head, int64_t ldh, int64_t m, int c, float* out, int64_t ldo, int out_col,
                     void* stream);
/* out = act(a + b) over `count` fp32 values (count % 4 == 0): the block's closing relu(x + res) (:109) */
int ptv3_add_act(const float* a, const float* b, int act, float* out, int64_t count, void* stream);

/* ---- Point Transformer V2 grouped vector attention, eval forward -------------------------------------
 * GroupedVectorAttention.forward after its three input projections (pointcept/models/point_transformer_v2/
 * point_transformer_v2m2_base.py:116-136, pe_bias = True, pe_multiplier = False) in one launch: both pointops.grouping
 * calls, linear_p_bias, weight_encoding, the softmax, the mask and the einsum.  q / k / v (n,c) fp32, xyz (n,3) fp32,
 * idx (n,ns) int32 (-1, or anything outside [0,n), = missing), out (n,c) fp32.  With j = idx[i,s], I = c / groups and every
 * PointBatchNorm folded to a per-channel (scale s, shift t) that also carries the bias of the Linear in front of it:
 *   pos = xyz[j] - xyz[i]                                  (0 where j is missing)
 *   h   = relu(s_p * (w_p1 pos) + t_p)                     w_p1 (c,3), s_p / t_p (c)
 *   peb = w_p2 h + b_p2                                    w_p2 (c,c), b_p2 (c)     v_mfma_f32_16x16x4_f32, w_p2 streamed
 *   r   = k[j] - q[i] + peb                                (k[j] = 0 where j is missing)
 *   w   = w_w2 relu(s_w * (w_w1 r) + t_w) + b_w2           w_w1 (groups,c), s_w / t_w (groups), w_w2 (groups,groups)
 *   w   = softmax over the ns slots, per group; then w = 0 where j is missing (:129-132: after the softmax, no
 *         renormalisation; the missing slot took part with pos = 0, k = v = 0, peb = MLP(0))
 *   out[i, g*I + t] = sum_s (v[j, g*I + t] + peb[s, g*I + t]) * w[s, g]
 * h, peb, r and w live in registers and LDS only.  c: a multiple of 8 in [8,512]; groups: a divisor of c, at most 64;
 * ns in [1,32]; 0 <= n < 2^31 (n = 0 returns PTV3_OK without a launch); anything else, a NULL pointer included, is
 * refused with PTV3_ERR_ARG before any launch.  fp32 arithmetic, fixed summation order, no atomics: bitwise
 * reproducible. */
int ptv3_gva_fwd(const float* q, const float* k, const float* v, const float* xyz, const int32_t* idx, int64_t n, int c,
                 int groups, int ns, const float* w_p1, const float* s_p, const float* t_p, const float* w_p2,
                 const float* b_p2, const float* w_w1, const float* s_w, const float* t_w, const float* w_w2,
                 const float* b_w2, float* out, void* stream);

/* ---- Point Transformer V2 grid pooling (GridPool.forward, :251-276; PARITY UNPINNED) --------------------
 * The reference computes the partition with torch_scatter.segment_csr and torch_geometric's voxel_grid (torch_cluster
 * grid_cluster), none of which is in its tree; their published semantics are restated here.
 * ptv3_grid_keys: start[b] (num_scenes,3) = per-axis minimum of scene b's coordinates (:255-263), cell = (int64)((coord -
 * start[b]) / size) per axis in fp32 (a subtraction, then a correctly rounded division: the two operations torch
 * performs), key[i] = b << 51 | cz << 34 | cy << 17 | cx: ascending keys are the rank order torch.unique gives
 * voxel_grid's ids (x fastest, batch slowest), so ptv3_argsort_i64(key, end_bit 63) + ptv3_pool_segments(key, order,
 * shift 0, batch) yield `cluster`, the sorted order, the segments and the pooled offsets.  offset: (num_scenes) int64
 * cumulative scene ends on the device; batch (n) int64 out; *bad (device, zeroed by the caller) is set to 1 when a
 * cell does not fit 17 bits.  1 <= num_scenes <= 4096.
 * ptv3_segment_mean3: out[j] = mean of coord over the members order[seg_start[j] .. seg_start[j+1]) (:272), summed in
 * that order.  The feature max (:273) is ptv3_pool_reduce's feature half. */
int ptv3_grid_keys(const float* coord, int64_t n, const int64_t* offset, int num_scenes, float size, float* start,
                   int64_t* key, int64_t* batch, int64_t* bad, void* stream);
int ptv3_segment_mean3(const float* coord, const int64_t* order, const int32_t* seg_start, int64_t n_out, float* out,
                       void* stream);

/* ---- Stratified Transformer (ST-v1m2) window attention, eval forward (fp32) -----------------------------
 * The reference (pointcept/models/stratified_transformer/stratified_transformer_v1m2_refine.py) builds [windows, k, k]
 * masks and an edge list of M (query, key) pairs per block (BasicLayer.forward, :388-450) and attends over it with
 * pointops2's attention_step1_v2 / dot_prod_with_idx_v3 / attention_step2_with_rel_pos_value_v2 and a scatter_softmax
 * (WindowAttention.forward, :157-216; libs/pointops2/src/attention_v2, rpe_v2).  Every query of one (small window,
 * large window) pair has the same keys, so the plan here is a list of GROUPS and nothing per edge exists:
 *   q_ptr (G+1) / q_rows (n):  the rows of each group - every point is a query of exactly one group; a group is the
 *                              set of points that share a small window AND a large window
 *   k_ptr (G+1) / k_rows:      its keys - all rows of its small window, then the sampled rows of its large window that
 *                              lie in another small window.
 * ptv3_strat_cell_keys replaces the four grid_sample calls (:373-385): small cell = trunc(((x + s) - min) / w), large
 * cell = trunc(((x + 2 s) - min) / 2w), s = w / 2 in shifted blocks and 0 otherwise, each evaluated in fp32 operation by
 * operation as voxel_grid does and NEVER derived from the other (in shifted blocks a small window straddles two large
 * ones); coord_min (3) on the device is the batch-wide minimum (:372).  Two keys per point:
 *   key_small = scene << 51 | small cell (9 bits per axis) << 24 | large cell (8 bits per axis)
 *   key_large = scene << 51 | large cell << 27 | small cell
 * *bad (device, zeroed by the caller) is set when a cell does not fit.  ptv3_argsort_i64(key, end_bit 63) of each and
 * ptv3_pool_segments then give: from key_small, shift 0: q_rows = order_s and q_ptr; shift 24: the small windows' runs
 * c_ptr with cell_of (n); from key_large, shift 0: the same groups' runs lg_ptr in order_l with lgroup_of (n); shift 27:
 * the large windows' runs w_ptr with window_of (n).
 * ONE DELIBERATE DIFFERENCE: in shifted blocks the reference excludes sparse keys by trunc((x - min + w/2) / w) (:423),
 * which associates differently from voxel_grid's ((x + w/2) - min) / w; a point within rounding of a cell face can then be
 * a key twice.  Here the voxel_grid expression serves both uses.
 * ptv3_strat_key_count: count[g] for g < *n_groups (device), 0 for the other g < n.  sampled (n) uint8 marks down_idx;
 * sampled_prefix (n+1) int32 = exclusive prefix sum of sampled[order_l[.]].  The caller scans count into k_ptr, reads the
 * totals once, and ptv3_strat_key_fill writes s_rows (number of sampled rows) and k_rows. */
int ptv3_strat_cell_keys(const float* coord, int64_t n, const int32_t* offset, int num_scenes, const float* coord_min,
                         float window, int shifted, int64_t* key_small, int64_t* key_large, int32_t* bad, void* stream);
int ptv3_strat_key_count(const int32_t* q_ptr, const int64_t* order_s, const int64_t* cell_of, const int32_t* c_ptr,
                         const int64_t* lgroup_of, const int32_t* lg_ptr, const int64_t* window_of, const int32_t* w_ptr,
                         const int32_t* sampled_prefix, const int32_t* n_groups, int64_t n, int32_t* count, void* stream);
int ptv3_strat_key_fill(const int32_t* q_ptr, const int64_t* order_s, const int64_t* cell_of, const int32_t* c_ptr,
                        const int64_t* lgroup_of, const int32_t* lg_ptr, const int64_t* window_of, const int32_t* w_ptr,
                        const int64_t* order_l, const uint8_t* sampled, const int32_t* sampled_prefix, int64_t n,
                        int64_t n_groups, const int32_t* k_ptr, int32_t* s_rows, int32_t* k_rows, void* stream);
/* relative_position_index (:163-169) of m pairs: out (m,3) int32 =
 *   trunc((round((x_i - x_j) * 1e5) / 1e5 + 2 window - 1e-4) / quant), clamped to [0, table_rows),
 * bit for bit what torch's CPU kernels give in fp32 (one rounding per operation, IEEE division, round-half-even); the
 * same device function serves ptv3_strat_attn_fwd.  Used by the edge composition and by tests. */
int ptv3_strat_rel_index(const float* coord, const int32_t* qi, const int32_t* kj, int64_t m, float window, float quant,
                         int table_rows, int32_t* out, void* stream);
/* One launch for WindowAttention.forward between qkv and proj (:157-220), with qs = scale * q:
 *   e_ij  = qs_i . k_j + sum_a ( qs_i . Tq[r_a,h,:,a] + k_j . Tk[r_a,h,:,a] )
 *   out_i = sum_j softmax_j(e_ij) ( v_j + sum_a Tv[r_a,h,:,a] )        over the keys j of i's group
 * q, k, v: rows of `ld` floats (views into the qkv projection), head h at [16 h, 16 h + 16); coord (n,3); tq / tk / tv:
 * the (2L, heads, 16, 3) tables repacked axis-major to (3, table_rows, heads, 16); out (n, heads, 16), written for the
 * plan's query rows only.  head_dim 16 and 1 <= table_rows <= 80 (ptv3_strat_attn_capable), anything else is refused
 * with PTV3_ERR_ARG before a launch.  One wave per (group, head); keys stream through in chunks of 16 with a running
 * maximum and sum; all products on v_mfma_f32_16x16x4_f32; fp32, no atomics, bitwise reproducible. */
int ptv3_strat_attn_capable(int heads, int head_dim, int table_rows);
int ptv3_strat_attn_fwd(const float* q, const float* k, const float* v, int64_t ld, const float* coord, const float* tq,
                        const float* tk, const float* tv, const int32_t* q_ptr, const int32_t* q_rows,
                        const int32_t* k_ptr, const int32_t* k_rows, int64_t n_groups, int heads, int head_dim,
                        int table_rows, float scale, float window, float quant, float* out, void* stream);
/* torch_points_kernels.ball_query(radius, max_neighbor, x, x, mode="partial_dense", batch_x, batch_x)[0] as the model
 * calls it (:703-711; the package is not in the reference tree: PARITY UNPINNED).  idx (n, max_neighbor) int64: the first
 * max_neighbor rows j of i's own scene, in index order, with |x_i - x_j|^2 < radius^2 (i itself included), then -1. */
int ptv3_ball_query(const float* xyz, const int32_t* offset, int num_scenes, int64_t n, float radius, int max_neighbor,
                    int64_t* idx, void* stream);

/* ---- OctFormer (pointcept/models/octformer/octformer_v1m1_base.py; ocnn and dwconv are not in the reference tree:
 * PARITY UNPINNED) -------------------------------------------------------------------------------------------------
 * Leaf keys of ocnn's Octree.build_octree (:598-604): p = coord / scale_factor, cell = floor((p + 1) * 2^(depth-1)) per
 * axis in fp32 (one rounding per operation, IEEE division); key = scene << 48 | interleave(cell) with x in the highest
 * bit of each triple, then y, then z.  coord (n,3) fp32; offset (num_scenes) int32 cumulative scene ends; depth in
 * [1,16]; key (n) int64.  flag (1) int32, zeroed by the caller: set to 1 when some p lies outside -1 <= p < 1 (that
 * point's cell is clamped into the grid; the caller reads the flag with the node counts and raises).  The nodes of depth
 * d are then the runs of ptv3_argsort_i64(key, end_bit 63) + ptv3_pool_segments(key, order, 3*(depth-d)). */
int ptv3_octree_keys(const float* coord, const int32_t* offset, int num_scenes, int64_t n, float scale_factor, int depth,
                     int64_t* key, int32_t* flag, void* stream);
/* OctreeAttention.forward between the qkv and proj linears (:230-257) in one launch, without the padded copy, the
 * (patches, K, K) mask or the (patches, K, K, 3, H) table gather.  qkv (n_t, 3c) fp32 in node order, head h of q / k / v at
 * columns [h hd, (h+1) hd) of its third; xyz (n_t, 3) int32 node coordinates; batch (n_t) int32 scene ids; rpe_table
 * (3*(2*pos_bnd+1), heads) fp32; out (n_t, c) fp32 in node order.  Token j of patch d of group g is row
 * g*patch*dilation + j*dilation + d; for a query i and a key j of one patch
 *   logit_ij = (scale q_i) . k_j + sum_axis rpe_table[axis*(2b+1) + clamp(x_i - x_j, -b, b) + b][h],   b = pos_bnd,
 * and out_i = sum_j softmax_j(logit_ij) v_j over the keys j of i's scene.  The reference adds -1e3 to the keys of other
 * scenes and of the padding rows at or past n_t; exp of that is 0 in fp32 for logits of ordinary size, so the kernel
 * SKIPS those keys.  Rows at or past n_t are neither read nor written.
 * Covered (ptv3_octree_attn_capable): c / heads in {16, 32}, 1 <= patch <= 32, dilation >= 1; with pos_bnd <= 127.
 * Anything else: PTV3_ERR_UNSUPPORTED (a shape the kernel does not cover) or PTV3_ERR_ARG (a malformed call) before any
 * launch.  One wave per (patch, head), fp32 fused multiply-adds in a fixed order, 16-byte vector stores, no atomics:
 * bitwise reproducible. */
int ptv3_octree_attn_capable(int c, int heads, int patch, int dilation);
int ptv3_octree_attn_fwd(const float* qkv, const int32_t* xyz, const int32_t* batch, const float* rpe_table, float* out,
                         int64_t n_t, int c, int heads, int patch, int dilation, int pos_bnd, float scale, void* stream);
/* cpe(data) + data of OctFormerBlock.forward in eval (:143-160, :310): dwconv.OctreeDWConv over the 27-tap table with the
 * BatchNorm1d folded, plus the residual:
 *   out[i][ch] = x[i][ch] + (sum_t w[t][ch] x[nbr[i][t]][ch]) * bn_scale[ch] + bn_shift[ch]
 * x, out (n, c) fp32, out != x; w (27, c) fp32 (the (27, 1, c) parameter); nbr (n, 27) int32, tap (dx+1)*9 + (dy+1)*3 +
 * (dz+1), an entry outside [0, n) is an absent tap; c % 4 == 0 (16-byte accesses), else PTV3_ERR_ARG.  Taps are summed in
 * tap order: bitwise reproducible. */
int ptv3_octree_dwconv(const float* x, const float* w, const int32_t* nbr, const float* bn_scale, const float* bn_shift,
                       float* out, int64_t n, int c, void* stream);

/* ---- segmentation losses -------------------------------------------------------------------------
 * A row is VALID when labels[i] != ignore_index and 0 <= labels[i] < C; every other row is ignored (the reference
 * faults on an out-of-range label).  logits (n, C) fp32 row-major, labels (n) int64; 2 <= C <= 1024, n * C < 2^31,
 * 16-byte aligned buffers, else PTV3_ERR_ARG before any launch.  Nothing is read back; no atomics; two runs on the same
 * input are bitwise equal.
 *
 * ptv3_lovasz_fwd: LovaszLoss(mode="multiclass").forward of pointcept/models/losses/lovasz.py:241-257, that is
 *   y_pred.softmax(1), _flatten_probas (:167-184), the per-class loop of _lovasz_softmax_flat (:118-164: labels.unique(),
 *   fg, errors, torch.sort, fg[perm], the dot) and _lovasz_grad (:22-33), without the host reads of unique(), of
 *   `fg.sum() == 0` and of the boolean-mask compaction.  Per class c: err_i = |fg_i - p_ic| over the valid rows, sorted
 *   descending (ties by point index: a stable radix sort of the inverted float bits, not-valid rows last); with
 *   F = the running foreground count at sorted position i (1-based), G = the class's foreground count, I = G - F,
 *   U = G + i - F, the weight is 1/U on a foreground row, I / (U (U - 1)) on a background row, 1 - I/U at i = 1 on a
 *   background row: jaccard[i] - jaccard[i-1] of :28-32 in closed form, evaluated in float64 from integers (the
 *   reference's fp32 difference of near-equal numbers is off by tens of percent at a few thousand rows).
 *   out[0] = loss_weight * mean over the classes with G > 0 of sum_i err_i g_i; 0 when no row is valid (the reference
 *   returns an empty tensor there).  weight (n, C) fp32 = g in point order, 0 on a row that is not valid (kept for the
 *   backward); order (C, n) int64 = the per-class sorted order; count (C + 1) int32 = G_c, then the number of present
 *   classes.  workspace: ptv3_lovasz_workspace_bytes(n, C), 16-byte aligned.  ptv3_lovasz_scan_tile(): positions per
 *   workgroup of the scan.  Launches: prep, the radix passes of ptv3_argsort_i64 (k = C, end_bit 33), tile count, tile
 *   scan, apply, finish.
 * ptv3_lovasz_bwd: autograd of the above (softmax backward with the weights held constant, as torch's sort/gather
 *   gives): dP_c = dloss[0] * loss_weight / n_present * weight[i, c] * (fg ? -1 : +1) for a present class, 0 otherwise;
 *   dlogits[i, j] = p_j (dP_j - sum_k p_k dP_k); zeros on a row that is not valid.  One launch.
 *
 * ptv3_focal_fwd / ptv3_focal_bwd: FocalLoss.forward of pointcept/models/losses/misc.py:123-172 (the multi-class
 *   sigmoid form) and its autograd.  Per element, t the one-hot target: s = sigmoid(x), q = (1 - s) t + s (1 - t),
 *   a = alpha[c] t + (1 - alpha[c])(1 - t), bce = max(x, 0) - x t + log1p(exp(-|x|)), L = a q^gamma bce.
 *   out[0] = loss_weight * sum L over the valid rows, divided by n_valid * C with mean != 0 (:168-169); with mean == 0
 *   the plain sum (the reference calls a missing method there, :170-171).  0 when no row is valid (:148-149).
 *   nvalid[0] int32 = n_valid.  alpha (C) fp32 on the device; gamma >= 0.  Two launches (fixed chunks -> slab, one
 *   finishing workgroup in float64).  workspace: ptv3_focal_workspace_bytes(n, C), 16-byte aligned.
 *   bwd: dlogits = dloss[0] * loss_weight (/ (n_valid C)) * a q^gamma (gamma (1 - q)(1 - 2t) bce + (s - t)), zeros on a
 *   row that is not valid.  One launch. */
int ptv3_lovasz_scan_tile(void);
size_t ptv3_lovasz_workspace_bytes(int64_t n, int C);
int ptv3_lovasz_fwd(const float* logits, const int64_t* labels, int64_t n, int C, int64_t ignore_index,
                    float loss_weight, float* out, float* weight, int64_t* order, int32_t* count, void* workspace,
                    size_t workspace_bytes, void* stream);
int ptv3_lovasz_bwd(const float* dloss, const float* logits, const int64_t* labels, const float* weight,
                    const int32_t* count, int64_t n, int C, int64_t ignore_index, float loss_weight, float* dlogits,
                    void* stream);
size_t ptv3_focal_workspace_bytes(int64_t n, int C);
int ptv3_focal_fwd(const float* logits, const int64_t* labels, const float* alpha, int64_t n, int C,
                   int64_t ignore_index, float gamma, float loss_weight, int mean, float* out, int32_t* nvalid,
                   void* workspace, size_t workspace_bytes, void* stream);
int ptv3_focal_bwd(const float* dloss, const float* logits, const int64_t* labels, const float* alpha,
                   const int32_t* nvalid, int64_t n, int C, int64_t ignore_index, float gamma, float loss_weight, int mean,
                   float* dlogits, void* stream);

/* ---- PointGroup (pointcept/models/point_group/point_group_v1m1_base.py, libs/pointgroup_ops; the CUDA library cannot be
 * built for the fixtures: PARITY WITH pointgroup_ops UNPINNED) ----------------------------------------------------------
 * All entry points are fp32 / int32.  The ball query and the clustering share one workspace layout,
 * ptv3_pg_workspace_bytes(n) bytes, 16-byte aligned; n <= 2 000 000 (n * 1000 list entries fit an int32), at most 32767
 * scenes.  Both lay the points over a grid of edge 1.01 * radius (the 1 % covers the fp32 rounding of a cell position),
 * sort them by cell with ptv3_argsort_i64 and visit, per point, 9 runs of the sorted order.
 *
 * ptv3_pg_ballquery_batch_p: ballquery_batch_p of libs/pointgroup_ops/src/bfs_cluster_kernel.cu:16-91 and the retry
 *   loop of functions/functions.py:26-35.  The neighbours of point i are the rows k of its own scene with
 *   d2 = (xi-xk)^2 + (yi-yk)^2 + (zi-zk)^2 < radius^2 (:37-38, one fp32 rounding per operation, i included), in ascending
 *   k, at most the first 1000 (:21, :39-44).  start_len (n, 2) = (start, count); idx = the lists back to back.  The
 *   reference hands `start` out by atomicAdd in arrival order (:49); here start is the exclusive scan of count by point
 *   index - one of the reference's possible outputs, and bitwise repeatable.  batch_idxs (n) may be NULL (the scene is
 *   then found in batch_offsets); batch_offsets (num_scenes + 1) starts with 0.  Two calls on one workspace:
 *     idx == NULL: count pass, scan, start_len; *n_active (host) receives the number of list entries (one
 *                  synchronisation).  No meanActive retry: the count sizes idx exactly.
 *     idx != NULL: fills idx (*n_active entries) from the state the first call left in the workspace.  One wave per
 *                  point: up to 1000 hits are gathered from the 9 runs and put in index order in LDS; a point with more
 *                  scans its scene in index order like the reference and stops at 1000, so it keeps the 1000 lowest.
 * ptv3_pg_cluster: ballquery_batch_p + bfs_cluster (bfs_cluster.cpp:53-137) without the lists, the copy and the host
 *   search.  xyz (n, 3) the compacted centres, label (n), offsets (num_scenes + 1) from 0.  Every point counts all its
 *   neighbours and unions itself with each same-label neighbour of smaller index; a union hooks the larger root under
 *   the smaller by compare-and-swap (the only atomics), so a component's root is its smallest member whichever thread
 *   wins.  Components of size >= min_points are written ordered by smallest member, members ascending:
 *   cluster_idxs (., 2) = (cluster, point), cluster_offsets (clusters + 1); both are sized by the caller for the worst
 *   case, (n, 2) and (n + 1).  record_host[4] = clusters, list entries, 1 when a point has more than 1000 neighbours,
 *   clusters with more than propose_points members; it is read back once, the call's only synchronisation.  With the
 *   flag set the reference's lists would be cut and its graph directed, which a union cannot follow: the call returns
 *   PTV3_PG_TRUNCATED and the caller takes ptv3_pg_ballquery_batch_p + ptv3_pg_bfs_cluster_host.
 * ptv3_pg_bfs_cluster_host: find_cc / get_clusters / fill_cluster_idxs_ of bfs_cluster.cpp:53-111 on host arrays, from
 *   the algorithm: directed lists, seeds in ascending index, members in discovery order.  cluster_idxs (n, 2) and
 *   cluster_offsets (n + 1) sized for the worst case; counts[2] = clusters, list entries.  Returns 1 on a bad argument,
 *   2 when a list or an entry points outside the arrays.  Touches no GPU.
 * ptv3_pg_proposals: point_group_v1m1_base.py:145-174 on the device.  Keeps the clusters with MORE than propose_points
 *   members (:154; min_points above is >=), num_proposals of them as the caller knows from the record or the offsets.
 *   pred_classes (P) int64 = segment_pred of the cluster's first member, pred_scores (P) = the mean over the members of
 *   prob[row, class] (thread t of 256 adds members t, t + 256, ... in order, then a fixed tree: repeatable),
 *   pred_masks (P, n_rows) int32.  row_map (n_map, optional): cluster_idxs[:, 1] index it and it gives the row (:141-143).
 *   slot: (num_clusters) int32 scratch.  No atomics, no synchronisation. */
#define PTV3_PG_TRUNCATED 16
size_t ptv3_pg_workspace_bytes(int64_t n);
int ptv3_pg_ballquery_batch_p(const float* xyz, const int32_t* batch_idxs, const int32_t* batch_offsets, int num_scenes,
                              int64_t n, float radius, int32_t* start_len, int32_t* idx, int64_t* n_active,
                              void* workspace, size_t workspace_bytes, void* stream);
int ptv3_pg_cluster(const float* xyz, const int32_t* label, const int32_t* offsets, int num_scenes, int64_t n,
                    float radius, int min_points, int propose_points, int32_t* cluster_idxs, int32_t* cluster_offsets,
                    int32_t* record_host, void* workspace, size_t workspace_bytes, void* stream);
int ptv3_pg_bfs_cluster_host(const int32_t* semantic_label, const int32_t* ball_query_idxs, int64_t n_active,
                             const int32_t* start_len, int64_t n, int threshold, int32_t* cluster_idxs,
                             int32_t* cluster_offsets, int32_t* counts);
int ptv3_pg_proposals(const int32_t* cluster_idxs, const int32_t* cluster_offsets, int num_clusters, int64_t sum,
                      const float* prob, int num_classes, const int64_t* segment_pred, const int64_t* row_map,
                      int64_t n_map, int64_t n_rows, int propose_points, int num_proposals, int64_t* pred_classes,
                      float* pred_scores, int32_t* pred_masks, int32_t* slot, void* stream);

/* ptv3_pg_head_eval: both heads of PointGroup and what eval derives from them (point_group_v1m1_base.py:66-67, :101-117)
 *   in one launch.  feat (n, C) fp32, C = 64 or 96, 1 .. 256 classes (ptv3_pg_head_eval_capable).  bias_pred (n, 3) =
 *   Linear(w2, b2)(relu(BatchNorm(Linear(w1, b1)(feat)))) with the running statistics (scale = weight / sqrt(var + eps),
 *   the reference builds the norm with eps 1e-3); logit (n, K) = Linear(w_seg, b_seg)(feat); prob = softmax(logit);
 *   segment_pred (n) int64 = the first maximum of logit (the reference takes it of prob, :105: the same index unless two
 *   probabilities round together); center (n, 3) = (coord + bias_pred) / voxel_size, one rounding per operation as
 *   torch's add and div (:102-103); keep (n) uint8 = segment_pred is none of ignore_host[0 .. num_ignore) (:107-117,
 *   at most 8).  Weights are torch's (out, in) row-major.  All weights are staged once per workgroup in LDS (151 KB at
 *   C = 96 with 256 classes); a workgroup then walks tiles of 8 rows.  fp32 fma chains in input-channel order, no atomics.
 * ptv3_pg_bias_loss_fwd: :75-89.  mask = instance != ignore_index, g = centroid - coord; out[0] = sum mask |p - g|_1 /
 *   (sum mask + 1e-8), out[1] = sum mask (-(p / (|p| + 1e-8)) . (g / (|g| + 1e-8))) / (sum mask + 1e-8), out[2] = the
 *   denominator (kept for the backward).  One launch of one workgroup: thread t of 1024 adds rows t, t + 1024, ... in
 *   that order in float64, then a fixed tree - a two-stage fixed-order reduction, no atomics, bitwise repeatable.  Both
 *   losses are 0 when no row is unmasked.
 * ptv3_pg_bias_loss_bwd: autograd of the two losses with respect to bias_pred (n, 3), one launch; dloss[2] = the
 *   gradients arriving at out[0] and out[1], on the device.  At p == 0 the gradient of |p| is 0 as torch.norm's is (so
 *   only the v / (|p| + eps) term is left), and sign(0) = 0 as torch.abs's; masked rows get 0. */
int ptv3_pg_head_eval_capable(int c, int num_classes);
int ptv3_pg_head_eval(const float* feat, const float* coord, int64_t n, int c, int num_classes, const float* w1,
                      const float* b1, const float* bn_weight, const float* bn_bias, const float* bn_mean,
                      const float* bn_var, float bn_eps, const float* w2, const float* b2, const float* w_seg,
                      const float* b_seg, float voxel_size, const int* ignore_host, int num_ignore, float* bias_pred,
                      float* logit, float* prob, int64_t* segment_pred, float* center, uint8_t* keep, void* stream);
int ptv3_pg_bias_loss_fwd(const float* bias_pred, const float* coord, const float* centroid, const int64_t* instance,
                          int64_t ignore_index, int64_t n, float* out, void* stream);
int ptv3_pg_bias_loss_bwd(const float* dloss, const float* bias_pred, const float* coord, const float* centroid,
                          const int64_t* instance, int64_t ignore_index, int64_t n, const float* fwd_out, float* dbias,
                          void* stream);

/* Head of the context-aware classifier, pointcept/models/context_aware_classifier/context_aware_classifier_v1m1_base.py
 * (csrc/cac.hip).  All tensors fp32 row-major, labels int64, offset (nb) int64 cumulative scene ends.  No atomics: two
 * runs are bitwise equal.  Nothing is read back by the host.
 * ptv3_cac_capable: the (K classes, C channels) the kernels cover: 2 <= K <= 256, 1 <= C <= 128 and every kernel's LDS
 *   need (the largest is 4 * (Kp * (C + 1) + 32 * (C + 1 + Kp)) bytes, Kp = K rounded up to 4) within 144 KiB.
 * ptv3_cac_proto_fwd: class prototypes, two weightings behind one accumulation scheme.
 *   logits != NULL (softmax form, :131-142 per scene of post_refine_proto_batch): p = softmax(logits[i]); with
 *     conf_thresh > 0 a point whose largest p is below it contributes nothing; proto (nb, K, C) =
 *     sum_i p[i, k] x[i] / (sum_i p[i, k] + 1e-7) over the points of a scene; den (nb, K) = sum_i p[i, k].
 *   labels != NULL (label form, :78-90 of get_adaptive_perspective, whole batch, offset and nb ignored): proto (1, K, C)
 *     = sum_{t_i = k} x[i] / (count_k + 1e-4); den (K) = count_k as fp32, count (K) int32.  A label outside [0, K) is
 *     ignored (-1 is the reference's).  A class is present when count_k > 0: no unique().
 *   A workgroup takes 2048 rows that never straddle a scene, the chunks of a scene are added in increasing order in
 *   float64.  workspace: ptv3_cac_proto_workspace_bytes(n, K, C, nb).  Rows past offset[nb - 1] belong to no scene.
 * ptv3_cac_proto_bwd: dx (n, C) = sum_k w[i, k] dproto[b, k] / (den[b, k] + eps), the weights recomputed (the logits
 *   carry no gradient: detach_pre_logits=True).  Rows that belong to no scene are not written.
 * ptv3_cac_cos_logits_fwd: get_pred (:66-71) times temp per scene: out (n, K) = temp * <y_i / max(|y_i|, 1e-12),
 *   q[b, k] / max(|q[b, k]|, 1e-12)>; q (nb, K, C), or (1, K, C) for every row with shared != 0 (offset ignored).  The
 *   normalised rows stay in LDS.  Forward only: training composes get_pred in torch.
 * ptv3_cac_distill_fwd: get_distill_loss (:153-199) at smoothness 0.5, eps 0.  out[0] = the loss (0 when no label lies
 *   in [0, K)), coef (K) = the backward's per-class factor 1 / ((n_present + 1e-4)(sum entropy_k + 1e-4)), count (K + 1)
 *   int32 = valid rows per class, then n_present.  An ignored row takes class 0 in the smoothed label as the
 *   reference's onehot * (1 - ignore_mask) does, and weighs nothing.  workspace: ptv3_cac_distill_workspace_bytes(n, K).
 * ptv3_cac_distill_bwd: dpred (n, K) in one launch; `soft` carries no gradient (:158). */
int ptv3_cac_capable(int K, int C);
size_t ptv3_cac_proto_workspace_bytes(int64_t n, int K, int C, int nb);
int ptv3_cac_proto_fwd(const float* x, const float* logits, const int64_t* labels, const int64_t* offset, int nb,
                       int64_t n, int K, int C, float conf_thresh, float* proto, float* den, int32_t* count,
                       void* workspace, size_t workspace_bytes, void* stream);
int ptv3_cac_proto_bwd(const float* dproto, const float* den, const float* logits, const int64_t* labels,
                       const int64_t* offset, int nb, int64_t n, int K, int C, float conf_thresh, float* dx,
                       void* stream);
int ptv3_cac_cos_logits_fwd(const float* y, const float* q, const int64_t* offset, int nb, int64_t n, int K, int C,
                            int shared, float temp, float* out, void* stream);
size_t ptv3_cac_distill_workspace_bytes(int64_t n, int K);
int ptv3_cac_distill_fwd(const float* pred, const float* soft, const int64_t* labels, int64_t n, int K, float* out,
                         float* coef, int32_t* count, void* workspace, size_t workspace_bytes, void* stream);
int ptv3_cac_distill_bwd(const float* dloss, const float* pred, const float* soft, const int64_t* labels,
                         const float* coef, int64_t n, int K, float* dpred, void* stream);

/* Language-guided head of Point Prompt Training in eval, pointcept/models/point_prompt_training/
 * point_prompt_training_v1m1_language_guided.py:98-107 (csrc/ppt_head.hip): h = W x + b (D wide, CLIP's text space),
 * seg_logits = exp(logit_scale) * (h / |h|) . E_v^T over the K valid class embeddings.  Nothing nonlinear lies between W
 * and E_v, so the caller collapses them once per weights (ptv3_hip.ops.ppt_head_collapse, float64 on the host, rounded
 * once): with the thin factorisation W = Q R, q = Q^T b, beta = |b - Q q|^2, M = W^T E_v^T, c = E_v b
 *   |h|^2 = |R x + q|^2 + beta (still a sum of squares; the Gram form x^T W^T W x loses half the digits and is not used),
 *   h . e_k = (M^T x + c)_k.
 * ptv3_ppt_head_fwd: x (n, C) fp32 row-major, 16-byte aligned; B (C, C + K) = [R^T | M] row-major; bias (C + K) =
 *   [q | c]; beta; s = exp(logit_scale).  out (n, K) = s * (x B + bias)[C:] / sqrt(|(x B + bias)[:C]|^2 + beta).  No
 *   division guard: a zero h gives NaN as the reference's 0 / 0 does.  Products on the fp32 matrix cores (exact fma
 *   chains); no atomics, two runs are bitwise equal.  Forward only: training composes the head in torch.
 * ptv3_ppt_head_capable: C a multiple of 16 in [16, 128], K in [1, 256].  Anything else is refused with
 *   ptv3_last_error set and nothing launched. */
int ptv3_ppt_head_capable(int C, int K);
int ptv3_ppt_head_fwd(const float* x, const float* B, const float* bias, float beta, float s, int64_t n, int C, int K,
                      float* out, void* stream);

/* Self-distillation loss of "Sonata-v1m1", pointcept/models/sonata/sonata_v1m1_base.py:267-291 and :443-454
 * (csrc/sonata_loss.hip).  x (nt, K) teacher logits and s (ns, K) student logits, row-major, fp32
 * (PTV3_F32) or bf16 (PTV3_BF16) each; idx_t / idx_s (M) the matched rows, int64 or int32 (`*_i32` != 0); idx_t may
 * repeat, idx_s is strictly increasing; an index outside its matrix is clamped to it.  With E = exp(x[idx_t] / T) the
 * reference's Sinkhorn-Knopp assignment (three row / column rounds) is target[m, k] = E[m, k] u[k] / d[m],
 * d[m] = sum_k E[m, k] u[k]; u is the result of three sweeps:
 *   u1 = 1 / (K A1), A1[k] = sum_m E[m, k];  u_{i+1} = 1 / (K A_{i+1}), A_{i+1}[k] = sum_m E[m, k] / (n d_i[m]),
 * n the number of pairs of all ranks.  exp is taken without a shift as the reference does: the logits are cosines and
 * T >= 0.04, so |x / T| <= 25; 1 / T and 1 / tau must be finite and positive.  For an even K the kernels access pairs of
 * columns (8 bytes in fp32, 4 in bf16) when x, s, u and ds start on such a boundary, and single columns otherwise: no
 * alignment is required, an aligned base is faster.  No atomics, two runs are bitwise equal,
 * nothing is read back by the host.  M = 0 is the caller's case (loss 0, nothing launched).
 * ptv3_sonata_capable: 2 <= K <= 4096.
 * ptv3_sonata_sk_pass: one sweep.  u == NULL: A[k] = sum_m E[m, k].  Otherwise A[k] = sum_m E[m, k] / (n_total d[m])
 *   with d from u in the same sweep; a row is read once.  A (K) is this rank's sum; u_next (K, may be NULL) =
 *   1 / (K A), for a caller that has nothing to reduce across ranks.  Workgroups take 64 pairs and store their K sums
 *   in the workspace (ptv3_sonata_sk_workspace_bytes(M, K)); the chunks are added in increasing order in float64.
 * ptv3_sonata_ce_fwd: loss_m = -sum_k target[m, k] (s[idx_s[m], k] / tau - lse[m]); the pairs of a scene of offset_s
 *   (nb cumulative ends of the student's scenes) are averaged, then the scenes 0 .. B - 1, B = 1 + the scene of the last
 *   pair: an empty scene below B counts with 0, the empty scenes behind it do not count (segment_coo(reduce="mean")
 *   with dim_size = index.max() + 1).  loss (1), d (M), lse (M), gscale (nb) = 1 / (count_b B) or 0, all fp32.
 *   workspace: ptv3_sonata_ce_workspace_bytes(M).
 * ptv3_sonata_ce_bwd: ds (ns, K) in the dtype of s: dloss[0] gscale[b] (softmax(s / tau) sum_k target - target) / tau in
 *   a matched row, exact zeros elsewhere; the target is recomputed from x, u and d.  The teacher gets no gradient. */
int ptv3_sonata_capable(int K);
size_t ptv3_sonata_sk_workspace_bytes(int64_t M, int K);
int ptv3_sonata_sk_pass(const void* x, int x_dtype, const void* idx_t, int idx_i32, int64_t nt, int64_t M, int K,
                        double inv_temp, const float* u, double n_total, float* A, float* u_next, void* workspace,
                        size_t workspace_bytes, void* stream);
size_t ptv3_sonata_ce_workspace_bytes(int64_t M);
int ptv3_sonata_ce_fwd(const void* x, int x_dtype, const void* idx_t, int idx_t_i32, int64_t nt, const void* s,
                       int s_dtype, const void* idx_s, int idx_s_i32, int64_t ns, int64_t M, int K, double inv_temp,
                       double inv_tau, const float* u, const int64_t* offset_s, int nb, float* loss, float* d, float* lse,
                       float* gscale, void* workspace, size_t workspace_bytes, void* stream);
int ptv3_sonata_ce_bwd(const float* dloss, const void* x, int x_dtype, const void* idx_t, int idx_t_i32, int64_t nt,
                       const void* s, int s_dtype, const void* idx_s, int idx_s_i32, int64_t ns, int64_t M, int K,
                       double inv_temp, double inv_tau, const float* u, const float* d, const float* lse,
                       const int64_t* offset_s, int nb, const float* gscale, void* ds, void* stream);

/* Image branch of "Concerto-v1m1", pointcept/models/concerto/concerto_v1m1_base.py:529-573 and :781-845
 * (csrc/concerto.hip).  No atomics anywhere: every reduction runs in a fixed order, two runs are
 * bitwise equal; nothing is read back by the host.
 * ptv3_concerto_pool_corr: one pooling level of the pixel correspondences.  corr_in (n_in, V, 2) fp32, order (n_in) and
 *   seg_start (n_out + 1) of the pooling (its children in cluster order), out (n_out, V, 2) fp32.  Per cluster and view:
 *   count = children with BOTH entries != -1; sum over ALL children with every entry == -1 replaced by 0, elementwise;
 *   out = sum / count, or (-1, -1) when count == 0.  Sums in float64, rounded to fp32 once: the result does not depend
 *   on the order inside a segment.  An `order` entry outside [0, n_in) is skipped.
 * ptv3_concerto_pair_keys: key (R * V + 1) int64 of the pairs (r, v) in that order, r a position in `rows` (R feature
 *   rows, ascending), scene (R) the scene of each, img_base (ns) the first image of a scene.  A pair is valid when ANY of
 *   corr[rows[r], v] is != -1; its key is the patch (img_base[scene[r]] + v) * patch_h * patch_w + trunc(c0) * patch_w +
 *   trunc(c1), or n_patches when that lies outside [0, n_patches) (a violated precondition, kept in one bucket that the
 *   caller can see); an invalid pair and the extra last entry get PTV3_CONCERTO_NO_PATCH, above every patch.
 * ptv3_concerto_plan_finish: from the stable argsort `order` of the keys and its run starts seg_start (>= U + 1):
 *   patch_ids (U) = the key of each of the first U runs, pair_row (R * V) = rows[order[i] / V], the feature row of the
 *   i-th pair by (patch, r, v); entries behind seg_start[U] belong to no patch.
 * ptv3_concerto_patch_mean_fwd: mean (U, C) fp32, mean[j] = the mean of feat[pair_row[i]], seg_start[j] <= i <
 *   seg_start[j + 1], added in that order in fp32.  feat (n, C) fp32 (PTV3_F32) or bf16 (PTV3_BF16); a row outside
 *   [0, n) is clamped.  Rows are read 4 columns at a time when C is a multiple of 4 and feat 16-byte aligned.
 * ptv3_concerto_patch_mean_bwd: dfeat (n, C) in `dtype`, EVERY row written: the sum over v of dmean[slot[r * V + v]] /
 *   count[slot] (slot < U, v ascending) for the rows in `rows` (found by bisection), zeros elsewhere.  slot (>= R * V)
 *   is the run of each pair in (r, v) order.
 * ptv3_concerto_cos_*: a (U, D) fp32 / bf16, b (nb, D) fp32 / bf16 read at row patch_ids[j] (clamped to [0, nb)).  With
 *   shift != 0 both rows lose their mean over D.  cos[j] = a . b / (max(|a|, 1e-6) max(|b|, 1e-6)), loss[0] =
 *   10 mean_j (1 - cos[j]) (rows added in two fixed-order stages in float64).  Means, centred rows, dot product and norms
 *   are float64.  stats (U, 4) fp32 = mean of a, mean of b, |a'|, |b'| of the shifted rows, for the caller to look at.
 *   bwd: da (U, D) in a's dtype = -10 dloss[0] / U (b' - (a' . b' / |a'|^2) a') / (max(|a'|, eps) max(|b'|, eps)), without
 *   the second term on a's eps branch; the statistics are formed again in float64 from the rows, which the kernel holds
 *   in registers (one pass over a and b); b gets no gradient.
 * ptv3_concerto_cos_capable: 1 <= D <= 2048 (a row lives in the registers of one wavefront). */
#define PTV3_CONCERTO_NO_PATCH 0x4000000000000000
int ptv3_concerto_pool_corr(const float* corr_in, const int64_t* order, const int32_t* seg_start, int64_t n_in,
                            int64_t n_out, int V, float* out, void* stream);
int ptv3_concerto_pair_keys(const float* corr, int64_t n, const int64_t* rows, const int64_t* scene, int64_t R, int V,
                            const int64_t* img_base, int ns, int patch_h, int patch_w, int64_t n_patches, int64_t* key,
                            void* stream);
int ptv3_concerto_plan_finish(const int64_t* key, const int64_t* order, const int32_t* seg_start, const int64_t* rows,
                              int64_t R, int V, int64_t U, int64_t* patch_ids, int64_t* pair_row, void* stream);
int ptv3_concerto_patch_mean_fwd(const void* feat, int dtype, int64_t n, int C, const int64_t* pair_row,
                                 const int32_t* seg_start, int64_t U, float* mean, void* stream);
int ptv3_concerto_patch_mean_bwd(const float* dmean, const int64_t* rows, const int64_t* slot, const int32_t* seg_start,
                                 int64_t n, int64_t R, int V, int64_t U, int C, void* dfeat, int dtype, void* stream);
int ptv3_concerto_cos_capable(int D);
int ptv3_concerto_cos_fwd(const void* a, int a_dtype, const void* b, int b_dtype, const int64_t* patch_ids, int64_t U,
                          int64_t nb, int D, int shift, float* cos, float* stats, float* loss, void* stream);
int ptv3_concerto_cos_bwd(const float* dloss, const void* a, int a_dtype, const void* b, int b_dtype,
                          const int64_t* patch_ids, int64_t U, int64_t nb, int D, int shift, void* da, void* stream);

/* ---- validation hooks: SemSegEvaluator / ClsEvaluator / InsSegEvaluator (csrc/evaluator.hip) -------------------------
 * Element types of the arrays these two entry points dispatch over, beside PTV3_F32 / PTV3_BF16. */
#define PTV3_F16 2
#define PTV3_I32 3
#define PTV3_I64 4
#define PTV3_U8 5 /* torch.uint8 and torch.bool */
/* ptv3_seg_confusion: output.max(1)[1], pred[inverse] and intersection_and_union_gpu of the reference's
 *   pointcept/engines/hooks/evaluator.py:39-46 / :141-152 and pointcept/utils/misc.py:53-65 as one counting pass.
 *   src is either logits (n, K) in PTV3_F32 / PTV3_BF16 / PTV3_F16 - the prediction of a row is then the LOWEST index
 *   among its maxima; a row with a NaN is out of contract - or the prediction (n) itself in PTV3_I32 / PTV3_I64.  target
 *   (m) PTV3_I32 / PTV3_I64.  With inverse (m) int64, element e is predicted by row inverse[e] (an entry outside [0, n) is
 *   counted nowhere); without it m == n.  Logits WITH an inverse take pred_ws (n) int32, else it may be NULL.
 *   counts (3, K) int64 = intersection, predicted area, target area, ADDED to what is there (union = predicted + target -
 *   intersection is the caller's).  An element whose target equals ignore_index takes ignore_index as its prediction; a
 *   value outside [0, K) falls in no bin of any of the three: the histc(bins=K, min=0, max=K-1) calls over integers.
 *   1 <= K <= PTV3_SEG_CONFUSION_MAX_K (the 3K-bin histogram lives in LDS); n, m < 2^31.  Integer atomics: bitwise equal
 *   from run to run.
 * ptv3_insseg_associate: the body of InsSegEvaluator.associate_instances (evaluator.py:309-341) for one scene, without
 *   the gathered copy of :577.  masks (P, nm) PTV3_I32 / PTV3_U8 / PTV3_I64, an entry is SET when != 0 (:317).  code (n)
 *   int32 per evaluated point: bits 0-30 the compact index of the point's counted ground-truth instance in [0, G), or G
 *   for none (a larger value is counted in no column); bit 31 set when the point's segment is ignored (void).
 *   col_start NULL: the evaluated cloud is the masks' own, n == nm, point j is column j.  col_start (nm + 1) int32: the
 *   evaluated cloud is another one (the nearest-neighbour map of :569-576, inverted by the caller): the points that read
 *   column j are col_start[j] .. col_start[j + 1] - 1 and `code` is stored in that order; a range is clipped to [0, n].
 *   Either way a row of masks is read once, in order.  Outputs, all int32 and all OVERWRITTEN: inter (P, G + 1)[p, g] =
 *   evaluated points of code g on set entries of p (:327-331), vert_count (P) = evaluated points on set entries (:318),
 *   void_inter (P) = those of them that are void (:319-321).  0 <= G <= PTV3_INSSEG_MAX_GT (the row's histogram lives in
 *   LDS); a row is cut into chunks of ptv3_insseg_chunk() entries, one workgroup each, and the result does not depend
 *   on the cut.  P == 0 or n == 0 launches nothing. */
#define PTV3_SEG_CONFUSION_MAX_K 1024
#define PTV3_INSSEG_MAX_GT 4095
int ptv3_seg_confusion(const void* src, int src_dtype, int64_t n, const int64_t* inverse, const void* target,
                       int target_dtype, int64_t m, int K, int64_t ignore_index, int64_t* counts, int32_t* pred_ws,
                       void* stream);
int ptv3_insseg_chunk(void);
int ptv3_insseg_associate(const void* masks, int mask_dtype, int64_t P, int64_t nm, const int32_t* col_start,
                          const int32_t* code, int64_t n, int G, int32_t* inter, int32_t* vert_count, int32_t* void_inter,
                          void* stream);

/* Modulation of every PDBatchNorm of "SpUNet-v1m3" at once (csrc/pdnorm.hip, DESIGN.md section 28;
 * pointcept/models/sparse_unet/spconv_unet_v1m3_pdnorm.py:63-74).  With a = SiLU(context) (Cc), layer l of width C_l has
 * W_l (2 C_l, Cc) and b_l (2 C_l), row-major fp32: rows [0, C_l) give shift, rows [C_l, 2 C_l) give scale (the order of
 * .chunk(2, dim=1)); gamma_l / beta_l (C_l) are the affine parameters of the active BatchNorm, NULL for 1 and 0.
 * `table` is a DEVICE array of L rows of PTV3_PDNORM_ROW int64 - the addresses of W_l, b_l, gamma_l, beta_l and the
 * active BatchNorm's running mean and variance (0 for NULL), then off_l = C_0 + .. + C_{l-1} and C_l; `widths` is the HOST
 * array of the same C_l, which is what is checked before anything is launched (the host never reads the device table).
 * Outputs are packed over sum(C_l) in layer order.
 * ptv3_pdnorm_fwd, one launch: scale = W[C:] a + b[C:], shift = W[:C] a + b[:C];
 *   fold == 0: out0 = gamma (1 + scale), out1 = beta (1 + scale) + shift - the weight / bias of a BatchNorm that
 *     computes BN_affine(x) (1 + scale) + shift; one_plus (or NULL) receives 1 + scale for the backward.
 *   fold != 0: additionally reads mean / var of the table (must not be NULL: the caller passes has_stats = 1 to say
 *     so) and writes out0 = s = gamma (1 + scale) / sqrt(var + eps), out1 = t = beta (1 + scale) + shift - mean s: the
 *     (bn_scale, bn_shift) pair of the conv epilogues.
 * ptv3_pdnorm_bwd, two launches (the second sums the slabs): from d_out0 = d gamma_eff, d_out1 = d beta_eff (packed)
 *   dshift = d_out1, dscale = d_out0 gamma + d_out1 beta, dgamma = d_out0 (1 + scale), dbeta = d_out1 (1 + scale)
 *   (dgamma / dbeta may be NULL), db (2 sum C) with layer l at 2 off_l = [dshift; dscale], dW (2 sum C, Cc) with layer l
 *   at row 2 off_l = [dshift; dscale] (x) a, dcontext (Cc) = SiLU'(context) . sum_l W_l^T [dshift; dscale].  The sum over
 *   channels goes through `partial` (ptv3_pdnorm_partial_rows(total) x Cc floats, fully overwritten) and a final sum in
 *   a fixed order: no atomics, two runs are bitwise equal.
 * Capable: 1 <= C_l <= 4096, 1 <= Cc <= 1024, 1 <= L <= 4096.  16-byte loads along Cc when Cc % 4 == 0 and W is 16-byte
 * aligned, 4-byte ones otherwise (decided per layer on the device; the results do not depend on it beyond rounding).
 * Anything else, a NULL pointer included, is refused with PTV3_ERR_ARG before any launch. */
#define PTV3_PDNORM_ROW 8 /* int64 entries per layer of `table`: &W, &b, &gamma, &beta, &mean, &var (0: NULL), off, C */
int ptv3_pdnorm_capable(int C, int Cc);
int ptv3_pdnorm_partial_rows(int64_t total);
int ptv3_pdnorm_fwd(const int64_t* table, const int32_t* widths, int L, int Cc, const float* context, int fold,
                    int has_stats, float eps, float* out0, float* out1, float* one_plus, void* stream);
int ptv3_pdnorm_bwd(const int64_t* table, const int32_t* widths, int L, int Cc, const float* context,
                    const float* d_out0, const float* d_out1, const float* one_plus, float* dW, float* db, float* dgamma,
                    float* dbeta, float* partial, float* dcontext, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PTV3_HIP_H */
