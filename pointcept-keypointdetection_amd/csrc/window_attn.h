// One description of a serialized window-attention call, shared by the ten C entry points (window_attn.hip: the five
// forwards, attn_bwd.hip: the five backwards) and by the callers inside the library (engine.hip, block_train.hip).
// An entry point fills the parts it exposes, names the parts it insists on, and calls window_attn_forward or
// window_attn_backward; a new argument of the operation is added here, in window_attn_validate, in the entry that
// exposes it and in ops._attn_check on the Python side.
#pragma once
#include "common.h"
#include "../../include/ptv3_hip.h"

namespace ptv3 {

constexpr int AB_MAX_TAB = 1024;  // 3 * (2 * pos_bnd + 1) entries of one head's table column held in LDS by the backward

struct WindowAttnCall {
  const void* qkv;                // (n, 3c)
  const int32_t* win_order;       // (n_pad)
  const int32_t* win_inverse;     // (n)
  void* out;                      // (n, c): written by the forward, read by the backward
  int64_t n, n_pad;
  int c, heads, patch;            // patch: slots of a uniform window, or the longest ragged one (max_seqlen)
  float scale;
  int dtype;
  hipStream_t stream;
  // backward only
  const void* dout;
  void* dqkv;
  void* workspace;
  size_t workspace_bytes;
  // optional: ragged windows [cu_seqlens[w], cu_seqlens[w+1]) and the sum of their squared lengths (profiler's flops)
  const int32_t* cu_seqlens;
  int num_windows;
  double sum_len_sq;
  // optional: dense bias (windows, heads, patch, patch), forward only
  const float* rpe_bias;
  // optional: RPE table lookup inside the kernel; dtable is the backward's table gradient
  const int32_t* grid_coord;
  const float* rpe_table;
  int pos_bnd;
  float* dtable;
  // optional: log2-domain log-sum-exp rows (n_pad, heads): written by the forward, read (never written) by the backward
  float* lse;
  // optional: attention dropout, 0 = none
  float p_drop;
  uint32_t seed;
  // filled by the callee: windows of the call, and whether the forward took the tiled kernel (profiler tag)
  int nwin;
  bool tiled;
};

// the arguments every entry point has; the optional parts start out absent
inline WindowAttnCall window_attn_call(const void* qkv, const int32_t* win_order, const int32_t* win_inverse, void* out,
                                       int64_t n, int64_t n_pad, int c, int heads, int patch, float scale, int dtype,
                                       void* stream) {
  WindowAttnCall a{};
  a.qkv = qkv; a.win_order = win_order; a.win_inverse = win_inverse; a.out = out;
  a.n = n; a.n_pad = n_pad; a.c = c; a.heads = heads; a.patch = patch; a.scale = scale; a.dtype = dtype;
  a.stream = (hipStream_t)stream;
  return a;
}

// what an entry point insists on beyond the common checks; name is the prefix of its messages
enum { WA_RAGGED_NO = 0, WA_RAGGED_OPTIONAL, WA_RAGGED_REQUIRED };
struct WindowAttnSpec {
  const char* name;
  int ragged;                     // NO: cu_seqlens is not looked at; REQUIRED: patch is reported as max_seqlen
  bool lse, rpe, drop;            // the part must be present
};

// Every host-side check of a call, in one order for all entries; backward adds the workspace check.  Sets a.nwin.
// *empty: n == 0, nothing to launch.  The forwards and the RPE backward answer an empty call before they look at the
// head dim, the other backwards look at the head dim first (what each entry has always done).
int window_attn_validate(WindowAttnCall& a, const WindowAttnSpec& spec, bool backward, bool* empty);
int window_attn_forward(WindowAttnCall& a, const WindowAttnSpec& spec);
int window_attn_backward(WindowAttnCall& a, const WindowAttnSpec& spec);

// (dtype, head_dim) -> f(TypeTag<T>{}, std::integral_constant<int, head_dim / 16>{}); validated calls only
template <typename F> inline int window_attn_dispatch(int dtype, int head_dim, F&& f) {
  int rc = PTV3_ERR_UNSUPPORTED;
  by_dtype(dtype, [&](auto t) {
    by_value<16, 32, 64>(head_dim, [&](auto HD) { rc = f(t, std::integral_constant<int, HD() / 16>{}); });
  });
  return rc;
}

}  // namespace ptv3
