"""Tensor-level wrappers over the C ABI (include/ptv3_hip.h).

torch supplies device memory and the current HIP stream; all arithmetic happens in libptv3_hip.so.
Every wrapper validates device / dtype / contiguity on the host before a pointer reaches a kernel.
"""
import ctypes
from types import SimpleNamespace

import torch

from .lib import lib, PTV3_F32, PTV3_BF16, ACT_NONE, ACT_GELU, ACT_RELU, ORDER_IDS  # noqa: F401
from .lib import PTV3_ERR_UNSUPPORTED, PTV3_PG_TRUNCATED
from .lib import PTV3_HASH_FNV as HASH_FNV, PTV3_HASH_RAVEL as HASH_RAVEL  # noqa: F401
from .lib import (PTV3_KP_ARGMAX as KP_ARGMAX, PTV3_KP_WEIGHTED as KP_WEIGHTED,  # noqa: F401
                  PTV3_KP_GT_MEAN as KP_GT_MEAN, PTV3_KP_GT_FIRST as KP_GT_FIRST)
from .lib import PTV3_CLS_HEAD_ROW_TILE as CLS_HEAD_ROW_TILE  # noqa: F401

_DT = {torch.float32: PTV3_F32, torch.bfloat16: PTV3_BF16}

_raw_stream = torch._C._cuda_getCurrentRawStream if hasattr(torch._C, "_cuda_getCurrentRawStream") else None


def _stream():
    """Raw hipStream_t of torch's current stream (the fast C accessor; ~20x cheaper than current_stream())."""
    if _raw_stream is not None:
        return _raw_stream(torch.cuda.current_device())
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return None if t is None else t.data_ptr()


def _chk(t, name, dtype=None, dim=None):
    if t is None:
        return
    if not t.is_cuda:
        raise RuntimeError(f"{name}: expected a GPU tensor (the PTv3 HIP path has no CPU fallback)")
    if not t.is_contiguous():
        raise RuntimeError(f"{name}: tensor must be contiguous")
    if dtype is not None and t.dtype not in (dtype if isinstance(dtype, tuple) else (dtype,)):
        raise TypeError(f"{name}: dtype {t.dtype}, expected {dtype}")
    if dim is not None and t.dim() != dim:
        raise RuntimeError(f"{name}: {t.dim()}-d tensor, expected {dim}-d")


def k_granule(dtype):
    """K (input-channel) granularity of ptv3_gemm: 16 bytes."""
    return 4 if dtype == torch.float32 else 8


def _dt(t):
    try:
        return _DT[t.dtype]
    except KeyError:
        raise TypeError(f"unsupported feature dtype {t.dtype} (float32 or bfloat16)")


# ---------------------------------------------------------------------------------------------
# serialization
# ---------------------------------------------------------------------------------------------
def sfc_encode(grid_coord, batch, depth, orders):
    """code (k, n) int64; replaces encode() of utils/serialization/default.py:9-24 for k orders."""
    _chk(grid_coord, "grid_coord", (torch.int32, torch.int64), 2)
    _chk(batch, "batch", torch.int64, 1)
    n = grid_coord.shape[0]
    ids = (ctypes.c_int * len(orders))(*[ORDER_IDS[o] for o in orders])
    code = torch.empty((len(orders), n), dtype=torch.int64, device=grid_coord.device)
    lib.check(lib.ptv3_sfc_encode(_p(grid_coord), int(grid_coord.dtype == torch.int64), _p(batch), n, int(depth),
                                  ids, len(orders), _p(code), _stream()), "ptv3_sfc_encode")
    return code


def argsort_codes(code, end_bit):
    """(order, inverse), both (k, n) int64: stable argsort of every row + its inverse permutation."""
    _chk(code, "code", torch.int64, 2)
    k, n = code.shape
    order = torch.empty_like(code)
    inverse = torch.empty_like(code)
    ws_bytes = lib.ptv3_argsort_workspace_bytes(k, n)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=code.device)
    lib.check(lib.ptv3_argsort_i64(_p(code), k, n, int(end_bit), _p(order), _p(inverse), _p(ws), ws_bytes,
                                   _stream()), "ptv3_argsort_i64")
    return order, inverse


def argsort_codes_rows(code, end_bit):
    """argsort_codes() through ptv3_argsort_i64_rows, the executor's form: (order, inverse, row_order), row_order (n)
    int32 = order[0], written by the sort's last pass."""
    _chk(code, "code", torch.int64, 2)
    k, n = code.shape
    ws_bytes = lib.ptv3_argsort_workspace_bytes(k, n)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=code.device)
    order = torch.empty_like(code)
    inverse = torch.empty_like(code)
    row_order = torch.empty(n, dtype=torch.int32, device=code.device)
    lib.check(lib.ptv3_argsort_i64_rows(_p(code), k, n, int(end_bit), _p(order), _p(inverse), _p(row_order), _p(ws),
                                        ws_bytes, _stream()), "ptv3_argsort_i64_rows")
    return order, inverse, row_order


def coord_max(grid_coord, state=None):
    """max(0, largest grid coordinate) as a (1,) int32 device tensor (the executor's depth read-back).  state: (2,)
    int32 zeros, left zero again by the kernel (the executor keeps one and never refills it)."""
    _chk(grid_coord, "grid_coord", (torch.int32, torch.int64), 2)
    _chk(state, "state", torch.int32, 1)
    if state is None:
        state = torch.zeros(2, dtype=torch.int32, device=grid_coord.device)
    out = torch.empty(1, dtype=torch.int32, device=grid_coord.device)
    lib.check(lib.ptv3_coord_max(_p(grid_coord), int(grid_coord.dtype == torch.int64), grid_coord.shape[0], _p(state),
                                 _p(out), _stream()), "ptv3_coord_max")
    return out


def plan_sizes(offset_host, patch):
    """(n_pad, windows, ragged, sum of len^2) of the pad plan (v3m1_base.py:114-170): a scene longer than `patch` is
    padded to a multiple of it, a shorter one stays ONE short window (ragged; only with enable_flash=True)."""
    prev, n_pad, nwin, ragged, sq = 0, 0, 0, False, 0
    for o in offset_host:
        cnt = o - prev
        prev = o
        w = (cnt + patch - 1) // patch
        nwin += w
        if cnt < patch:
            ragged = True
            n_pad += cnt
            sq += cnt * cnt
        else:
            n_pad += w * patch
            sq += w * patch * patch
    return n_pad, nwin, ragged, sq


def pad_plan(offset, offset_host, patch):
    """pad, unpad, cu_seqlens of SerializedAttention.get_padding_and_inverse (v3m1_base.py:114-170)."""
    _chk(offset, "offset", torch.int64, 1)
    n_pad, nwin, _, _ = plan_sizes(offset_host, patch)
    n = int(offset_host[-1])
    pad = torch.empty(n_pad, dtype=torch.int64, device=offset.device)
    unpad = torch.empty(n, dtype=torch.int64, device=offset.device)
    cu = torch.empty(nwin + 1, dtype=torch.int32, device=offset.device)
    lib.check(lib.ptv3_pad_plan(_p(offset), len(offset_host), n, n_pad, int(patch), _p(pad), _p(unpad), _p(cu),
                                _stream()), "ptv3_pad_plan")
    return pad, unpad, cu


def window_maps(order, inverse, pad, unpad):
    for t, nm in ((order, "order"), (inverse, "inverse"), (pad, "pad"), (unpad, "unpad")):
        _chk(t, nm, torch.int64, 1)
    n, n_pad = order.shape[0], pad.shape[0]
    wo = torch.empty(n_pad, dtype=torch.int32, device=order.device)
    wi = torch.empty(n, dtype=torch.int32, device=order.device)
    lib.check(lib.ptv3_window_maps(_p(order), _p(inverse), _p(pad), _p(unpad), n, n_pad, _p(wo), _p(wi), _stream()),
              "ptv3_window_maps")
    return wo, wi


def window_plan(order, inverse, offset, offset_host, patch, with_cu=False):
    """(win_order (k, n_pad), win_inverse (k, n)) int32 for all k orders in one launch [+ cu_seqlens (windows+1)]."""
    _chk(order, "order", torch.int64, 2)
    _chk(inverse, "inverse", torch.int64, 2)
    _chk(offset, "offset", torch.int64, 1)
    k, n = order.shape
    n_pad, nwin, _, _ = plan_sizes(offset_host, patch)
    wo = torch.empty((k, n_pad), dtype=torch.int32, device=order.device)
    wi = torch.empty((k, n), dtype=torch.int32, device=order.device)
    cu = torch.empty(nwin + 1, dtype=torch.int32, device=order.device) if with_cu else None
    lib.check(lib.ptv3_window_plan(_p(order), _p(inverse), _p(offset), len(offset_host), k, n, n_pad, int(patch),
                                   _p(wo), _p(wi), _p(cu), _stream()), "ptv3_window_plan")
    return (wo, wi, cu) if with_cu else (wo, wi)


def _attn_check(who, qkv, win_order, win_inverse, heads, patch, cu_seqlens=None, out=None, dout=None, lse=None,
                grid_coord=None, rpe_table=None, pos_bnd=0):
    """What every window-attention wrapper checks before a pointer reaches a kernel; a tensor the wrapper does not take
    stays None.  -> (n, c, n_pad, windows).  A new argument of the operation is checked here (csrc/window_attn.h)."""
    _chk(qkv, "qkv", (torch.float32, torch.bfloat16), 2)
    _chk(win_order, "win_order", torch.int32, 1)
    _chk(win_inverse, "win_inverse", torch.int32, 1)
    _chk(cu_seqlens, "cu_seqlens", torch.int32, 1)
    _chk(out, "out", qkv.dtype, 2)
    _chk(dout, "dout", qkv.dtype, 2)
    _chk(lse, "lse", torch.float32, 2)
    _chk(grid_coord, "grid_coord", torch.int32, 2)
    _chk(rpe_table, "rpe_table", torch.float32, 2)
    n, c3 = qkv.shape
    c, n_pad = c3 // 3, win_order.shape[0]
    bad = c * 3 != c3 or win_inverse.shape[0] != n
    bad |= cu_seqlens is not None and cu_seqlens.numel() < 2
    bad |= any(t is not None and tuple(t.shape) != (n, c) for t in (out, dout))
    bad |= grid_coord is not None and tuple(grid_coord.shape) != (n, 3)
    bad |= rpe_table is not None and tuple(rpe_table.shape) != (3 * (2 * pos_bnd + 1), heads)
    if bad:
        raise RuntimeError(f"{who}: shape mismatch")
    if lse is not None and tuple(lse.shape) != (n_pad, int(heads)):
        raise RuntimeError(f"{who}: lse must be (n_pad, heads)")
    # a patch the library will refuse (outside [1, 16384], or not dividing n_pad) is left to its message
    nwin = cu_seqlens.numel() - 1 if cu_seqlens is not None else n_pad // max(int(patch), 1)
    return n, c, n_pad, nwin


def window_attention(qkv, win_order, win_inverse, heads, patch, scale, rpe_bias=None):
    """softmax(scale q k^T) v per window with gather/scatter fused (v3m1_base.py:188-216)."""
    n, c, n_pad, nwin = _attn_check("window_attention", qkv, win_order, win_inverse, heads, patch)
    _chk(rpe_bias, "rpe_bias", torch.float32)
    if rpe_bias is not None and rpe_bias.numel() != nwin * heads * patch * patch:
        raise RuntimeError("window_attention: rpe_bias must be (n_pad/patch, heads, patch, patch)")
    out = torch.empty((n, c), dtype=qkv.dtype, device=qkv.device)
    lib.check(lib.ptv3_window_attn_fwd(_p(qkv), _p(win_order), _p(win_inverse), _p(out), n, n_pad, c, int(heads),
                                       int(patch), float(scale), _p(rpe_bias), _dt(qkv), _stream()),
              "ptv3_window_attn_fwd")
    return out


def window_attention_varlen(qkv, win_order, win_inverse, cu_seqlens, heads, max_seqlen, scale, sum_len_sq=0.0):
    """The enable_flash=True call site (v3m1_base.py:207-215): flash_attn_varlen_qkvpacked_func semantics over ragged
    windows [cu_seqlens[w], cu_seqlens[w+1]) of at most max_seqlen padded slots, gather / scatter fused."""
    n, c, n_pad, nwin = _attn_check("window_attention_varlen", qkv, win_order, win_inverse, heads, max_seqlen, cu_seqlens)
    out = torch.empty((n, c), dtype=qkv.dtype, device=qkv.device)
    lib.check(lib.ptv3_window_attn_varlen_fwd(_p(qkv), _p(win_order), _p(win_inverse), _p(cu_seqlens), nwin, _p(out), n,
                                              n_pad, c, int(heads), int(max_seqlen), float(scale), float(sum_len_sq),
                                              _dt(qkv), _stream()), "ptv3_window_attn_varlen_fwd")
    return out


def window_attention_any(qkv, win_order, win_inverse, heads, patch, scale, cu_seqlens=None, sum_len_sq=0.0):
    """Uniform windows (cu_seqlens None) or ragged ones (the pad plan's cu_seqlens)."""
    if cu_seqlens is None:
        return window_attention(qkv, win_order, win_inverse, heads, patch, scale)
    return window_attention_varlen(qkv, win_order, win_inverse, cu_seqlens, heads, patch, scale, sum_len_sq)


def window_attention_train(qkv, win_order, win_inverse, heads, patch, scale, cu_seqlens=None, sum_len_sq=0.0):
    """The training forward: window_attention_any() that also returns the log-sum-exp rows (n_pad, heads) fp32 the
    backward would otherwise recompute."""
    n, c, n_pad, nwin = _attn_check("window_attention_train", qkv, win_order, win_inverse, heads, patch, cu_seqlens)
    out = torch.empty((n, c), dtype=qkv.dtype, device=qkv.device)
    lse = torch.empty((n_pad, int(heads)), dtype=torch.float32, device=qkv.device)
    lib.check(lib.ptv3_window_attn_train_fwd(_p(qkv), _p(win_order), _p(win_inverse), _p(cu_seqlens), nwin, _p(out),
                                             _p(lse), n, n_pad, c, int(heads), int(patch), float(scale),
                                             float(sum_len_sq), _dt(qkv), _stream()), "ptv3_window_attn_train_fwd")
    return out, lse


def window_attention_train_bwd(qkv, out, dout, lse, win_order, win_inverse, heads, patch, scale, cu_seqlens=None):
    n, c, n_pad, nwin = _attn_check("window_attention_train_bwd", qkv, win_order, win_inverse, heads, patch, cu_seqlens,
                                    out, dout, lse)
    dqkv = torch.empty_like(qkv)
    nb = lib.ptv3_window_attn_bwd_workspace_bytes(n, n_pad, c, int(heads), _dt(qkv))
    ws = _ws(nb, qkv.device)
    lib.check(lib.ptv3_window_attn_train_bwd(_p(qkv), _p(out), _p(dout), _p(lse), _p(win_order), _p(win_inverse),
                                             _p(cu_seqlens), nwin, _p(dqkv), n, n_pad, c, int(heads), int(patch),
                                             float(scale), _dt(qkv), _p(ws), nb, _stream()), "ptv3_window_attn_train_bwd")
    return dqkv


def window_attention_drop(qkv, win_order, win_inverse, heads, patch, scale, p_drop, seed, cu_seqlens=None):
    """Training forward with attention dropout (:203 / :211): softmax over all pairs, kept pairs / (1 - p_drop) into the
    value sum; the keep mask is a hash of (query slot, head, key slot, seed) - see drop_keep_mask()."""
    n, c, n_pad, nwin = _attn_check("window_attention_drop", qkv, win_order, win_inverse, heads, patch, cu_seqlens)
    out = torch.empty((n, c), dtype=qkv.dtype, device=qkv.device)
    lib.check(lib.ptv3_window_attn_drop_fwd(_p(qkv), _p(win_order), _p(win_inverse), _p(cu_seqlens), nwin, _p(out), n,
                                            n_pad, c, int(heads), int(patch), float(scale), float(p_drop),
                                            int(seed) & 0xFFFFFFFF, _dt(qkv), _stream()), "ptv3_window_attn_drop_fwd")
    return out


def window_attention_drop_bwd(qkv, out, dout, win_order, win_inverse, heads, patch, scale, p_drop, seed, cu_seqlens=None):
    n, c, n_pad, nwin = _attn_check("window_attention_drop_bwd", qkv, win_order, win_inverse, heads, patch, cu_seqlens,
                                    out, dout)
    dqkv = torch.empty_like(qkv)
    nb = lib.ptv3_window_attn_bwd_workspace_bytes(n, n_pad, c, int(heads), _dt(qkv))
    ws = _ws(nb, qkv.device)
    lib.check(lib.ptv3_window_attn_drop_bwd(_p(qkv), _p(out), _p(dout), _p(win_order), _p(win_inverse), _p(cu_seqlens),
                                            nwin, _p(dqkv), n, n_pad, c, int(heads), int(patch), float(scale),
                                            float(p_drop), int(seed) & 0xFFFFFFFF, _dt(qkv), _p(ws), nb, _stream()),
              "ptv3_window_attn_drop_bwd")
    return dqkv


def drop_keep_mask(slot, head, key, heads, seed, p_drop):
    """Host restatement of csrc/common.h drop_keep: numpy integer arrays (broadcastable) of padded query slots, heads and
    key slots inside the window -> boolean keep mask.  For tests and for anyone who needs the mask a call used."""
    import numpy as np
    idv = ((np.asarray(slot, np.uint64) * np.uint64(heads) + np.asarray(head, np.uint64)) << np.uint64(14)) | np.asarray(key, np.uint64)
    lo = (idv & np.uint64(0xFFFFFFFF)).astype(np.uint64)
    hi = (idv >> np.uint64(32)).astype(np.uint64)
    m32 = np.uint64(0xFFFFFFFF)
    x = ((lo * np.uint64(0x9E3779B1)) & m32) ^ ((hi * np.uint64(0x85EBCA77)) & m32) ^ np.uint64(int(seed) & 0xFFFFFFFF)
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & m32
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846CA68B)) & m32
    x ^= x >> np.uint64(16)
    thr = np.uint64(min(4294967295, int(float(np.float32(p_drop)) * 4294967296.0)))
    return x >= thr


def window_attention_rpe(qkv, win_order, win_inverse, heads, patch, scale, grid_coord, rpe_table, pos_bnd):
    """window_attention() + the RPE bias looked up from the (3*(2*pos_bnd+1), heads) table inside the kernel.
    Returns None when the window does not fit the resident-window kernel (caller falls back to the dense bias)."""
    n, c, n_pad, _ = _attn_check("window_attention_rpe", qkv, win_order, win_inverse, heads, patch,
                                 grid_coord=grid_coord, rpe_table=rpe_table, pos_bnd=pos_bnd)
    out = torch.empty((n, c), dtype=qkv.dtype, device=qkv.device)
    rc = lib.ptv3_window_attn_rpe_fwd(_p(qkv), _p(win_order), _p(win_inverse), _p(out), n, n_pad, c, int(heads),
                                      int(patch), float(scale), _p(grid_coord), _p(rpe_table), int(pos_bnd), _dt(qkv),
                                      _stream())
    if rc == PTV3_ERR_UNSUPPORTED:
        return None
    lib.check(rc, "ptv3_window_attn_rpe_fwd")
    return out


# ---------------------------------------------------------------------------------------------
# sparse conv support + the implicit GEMM
# ---------------------------------------------------------------------------------------------
def subm_neighbors(indices, ksize, table=None):
    """(nbr (n, ksize^3) int32, table) for unique (n,4) int32 [b,x,y,z] sites."""
    _chk(indices, "indices", torch.int32, 2)
    n = indices.shape[0]
    if table is None:
        slots = lib.ptv3_subm_table_slots(n)
        table = torch.empty(slots * 12, dtype=torch.uint8, device=indices.device)
        lib.check(lib.ptv3_subm_build_table(_p(indices), n, _p(table), slots, _stream()), "ptv3_subm_build_table")
    slots = table.numel() // 12
    nbr = torch.empty((n, ksize ** 3), dtype=torch.int32, device=indices.device)
    lib.check(lib.ptv3_subm_neighbors(_p(indices), n, _p(table), slots, int(ksize), _p(nbr), _stream()),
              "ptv3_subm_neighbors")
    return nbr, table


def subm_neighbors_blocks(indices, ksize, table=None):
    """subm_neighbors() through the table of 4x4x4 blocks (ptv3_subm_build_block_table): the same nbr, bitwise."""
    _chk(indices, "indices", torch.int32, 2)
    n = indices.shape[0]
    if table is None:
        table = torch.empty(lib.ptv3_subm_block_table_bytes(n), dtype=torch.uint8, device=indices.device)
        lib.check(lib.ptv3_subm_build_block_table(_p(indices), n, _p(table), table.numel(), _stream()),
                  "ptv3_subm_build_block_table")
    nbr = torch.empty((n, ksize ** 3), dtype=torch.int32, device=indices.device)
    lib.check(lib.ptv3_subm_neighbors_blocks(_p(indices), n, _p(table), table.numel(), int(ksize), _p(nbr), _stream()),
              "ptv3_subm_neighbors_blocks")
    return nbr, table


def subm_sites_table(batch, grid_coord):
    """The executor's level-0 table build: (indices (n,4) int32, grid64 (n,3) int64, table).  One launch writes the
    sites and zero-fills the table (ptv3_subm_sites), ptv3_subm_build_block_table_zeroed builds it without a memset."""
    _chk(batch, "batch", torch.int64, 1)
    _chk(grid_coord, "grid_coord", (torch.int32, torch.int64), 2)
    n = grid_coord.shape[0]
    indices = torch.empty((n, 4), dtype=torch.int32, device=batch.device)
    grid64 = torch.empty((n, 3), dtype=torch.int64, device=batch.device)
    table = torch.empty(lib.ptv3_subm_block_table_bytes(n), dtype=torch.uint8, device=batch.device)
    lib.check(lib.ptv3_subm_sites(_p(batch), _p(grid_coord), int(grid_coord.dtype == torch.int64), n, _p(indices),
                                  _p(grid64), _p(table), table.numel(), _stream()), "ptv3_subm_sites")
    lib.check(lib.ptv3_subm_build_block_table_zeroed(_p(indices), n, _p(table), table.numel(), _stream()),
              "ptv3_subm_build_block_table_zeroed")
    return indices, grid64, table


def gemm(x, w, bias=None, nbr=None, kvol=1, row_order=None, bn_scale=None, bn_shift=None, act=ACT_NONE,
         res=None, res_index=None, dual=False, m=None):
    """out = epi(sum_d sum_c w[o][d][c] x[nbr[i][d]][c]); see ptv3_gemm in include/ptv3_hip.h.

    Returns out, or (out_pre_residual, out_with_residual) when dual=True."""
    _chk(x, "x", (torch.float32, torch.bfloat16), 2)
    _chk(w, "w", x.dtype)
    for t, nm in ((bias, "bias"), (bn_scale, "bn_scale"), (bn_shift, "bn_shift")):
        _chk(t, nm, torch.float32, 1)
    _chk(nbr, "nbr", torch.int32, 2)
    _chk(row_order, "row_order", torch.int32, 1)
    _chk(res, "res", x.dtype, 2)
    _chk(res_index, "res_index", torch.int32, 1)
    cin = x.shape[1]
    cout = w.shape[0]
    if w.numel() != cout * kvol * cin:
        raise RuntimeError(f"gemm: weight has {w.numel()} elements, expected {cout}x{kvol}x{cin}")
    if m is None:
        m = nbr.shape[0] if nbr is not None else x.shape[0]
    if nbr is not None and (nbr.shape[0] != m or nbr.shape[1] != kvol):
        raise RuntimeError("gemm: neighbour table shape mismatch")
    for t in (bias, bn_scale, bn_shift):
        if t is not None and t.numel() != cout:
            raise RuntimeError("gemm: epilogue vector length != cout")
    if res is not None:
        if res.shape[1] != cout or (res_index is None and res.shape[0] != m):
            raise RuntimeError("gemm: residual shape mismatch")
        if res_index is not None and res_index.shape[0] != m:
            raise RuntimeError("gemm: res_index length != m")
    if row_order is not None and row_order.shape[0] != m:
        raise RuntimeError("gemm: row_order length != m")
    out = torch.empty((m, cout), dtype=x.dtype, device=x.device)
    out2 = torch.empty_like(out) if dual else None
    dt = _dt(x)
    ws_bytes = lib.ptv3_gemm_workspace_bytes(m, cin, cout, int(kvol), dt)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device) if ws_bytes else None
    lib.check(lib.ptv3_gemm(_p(x), _p(w), _p(out), m, cin, cout, int(kvol), _p(nbr), _p(row_order), _p(bias),
                            _p(bn_scale), _p(bn_shift), int(act), _p(res), _p(res_index), _p(out2), dt, _p(ws),
                            ws_bytes, _stream()), "ptv3_gemm")
    return (out, out2) if dual else out


def stem_conv_blocks(x, w, indices, table, ksize=5, bias=None, row_order=None, bn_scale=None, bn_shift=None, act=ACT_NONE,
                     out=None):
    """gemm(x, w, nbr=subm_neighbors_blocks(indices, ksize, table)[0], kvol=ksize^3, ...) without the neighbour table
    (ptv3_stem_conv_blocks): a tile resolves its neighbour rows from the block table into LDS.  Byte-equal to that call.
    out: an (n, cout) tensor to write into (tests pre-fill it to see a skipped store)."""
    _chk(x, "x", (torch.float32, torch.bfloat16), 2)
    _chk(w, "w", x.dtype)
    for t, nm in ((bias, "bias"), (bn_scale, "bn_scale"), (bn_shift, "bn_shift")):
        _chk(t, nm, torch.float32, 1)
    _chk(indices, "indices", torch.int32, 2)
    _chk(table, "table", torch.uint8, 1)
    _chk(row_order, "row_order", torch.int32, 1)
    n, cin = x.shape
    cout = w.shape[0]
    if indices.shape[0] != n or indices.shape[1] != 4:
        raise RuntimeError("stem_conv_blocks: indices must be (n, 4) for the n rows of x")
    if w.numel() != cout * int(ksize) ** 3 * cin:
        raise RuntimeError(f"stem_conv_blocks: weight has {w.numel()} elements, expected {cout}x{int(ksize) ** 3}x{cin}")
    for t in (bias, bn_scale, bn_shift):
        if t is not None and t.numel() != cout:
            raise RuntimeError("stem_conv_blocks: epilogue vector length != cout")
    if row_order is not None and row_order.shape[0] != n:
        raise RuntimeError("stem_conv_blocks: row_order length != n")
    if out is None:
        out = torch.empty((n, cout), dtype=x.dtype, device=x.device)
    _chk(out, "out", x.dtype, 2)
    if tuple(out.shape) != (n, cout):
        raise RuntimeError("stem_conv_blocks: out must be (n, cout)")
    lib.check(lib.ptv3_stem_conv_blocks(_p(x), _p(w), _p(out), n, cin, cout, int(ksize), _p(indices), _p(table),
                                        table.numel(), _p(row_order), _p(bias), _p(bn_scale), _p(bn_shift), int(act),
                                        _dt(x), _stream()), "ptv3_stem_conv_blocks")
    return out


def halo_plan_shape():
    """(T, CAP): sites per tile and the most distinct neighbour rows a tile may have on the fast path."""
    t, cap = ctypes.c_int(0), ctypes.c_int(0)
    lib.check(lib.ptv3_halo_plan_shape(ctypes.byref(t), ctypes.byref(cap)), "ptv3_halo_plan_shape")
    return t.value, cap.value


def halo_plan(nbr, row_order=None):
    """Halo plan of a 27-tap neighbour table (ptv3_halo_plan_build): (plan, counts, rows, slots).

    plan is the opaque byte tensor conv_halo takes; the other three are views into it: counts (tiles,) int32 distinct
    neighbour rows per tile of T consecutive sites of row_order (> CAP: the tile takes the slow path), rows (tiles, CAP)
    int32 of which the first min(count, CAP) per tile are written, slots (tiles, T, 27) int16 with -1 (0xFFFF) = absent."""
    _chk(nbr, "nbr", torch.int32, 2)
    _chk(row_order, "row_order", torch.int32, 1)
    m = nbr.shape[0]
    if nbr.shape[1] != 27:
        raise RuntimeError("halo_plan: the neighbour table must have 27 taps")
    if row_order is not None and row_order.shape[0] != m:
        raise RuntimeError("halo_plan: row_order length != m")
    t, cap = halo_plan_shape()
    tiles = (m + t - 1) // t
    nbytes = lib.ptv3_halo_plan_bytes(m)
    plan = torch.empty(nbytes, dtype=torch.uint8, device=nbr.device)
    lib.check(lib.ptv3_halo_plan_build(_p(nbr), _p(row_order), m, _p(plan), nbytes, _stream()), "ptv3_halo_plan_build")
    cb = (tiles * 4 + 15) // 16 * 16
    rb = tiles * cap * 4
    counts = plan[:tiles * 4].view(torch.int32)
    rows = plan[cb:cb + rb].view(torch.int32).view(tiles, cap)
    slots = plan[cb + rb:cb + rb + tiles * t * 27 * 2].view(torch.int16).view(tiles, t, 27)
    return plan, counts, rows, slots


def conv_halo_policy(m, c, dtype):
    """Whether the executor runs the c -> c 3^3 conv of m rows through conv_halo (PTV3_CONV_HALO)."""
    return bool(lib.ptv3_conv_halo_policy(int(m), int(c), int(c), 27, _DT[dtype]))


def conv_halo(x, w, nbr, plan, bias=None, row_order=None, bn_scale=None, bn_shift=None, act=ACT_NONE, res=None,
              res_index=None, dual=False, out=None):
    """gemm(x, w, nbr=nbr, kvol=27, ...) for cin = cout in {32, 64} with the tile's neighbour rows held in LDS
    (ptv3_conv_halo); plan = halo_plan(nbr, row_order)[0].  Bitwise the result of the single-pass 64-point tile.
    out: an (m, c) tensor to write into (tests pre-fill it to see a skipped store)."""
    _chk(x, "x", (torch.float32, torch.bfloat16), 2)
    _chk(w, "w", x.dtype)
    for t, nm in ((bias, "bias"), (bn_scale, "bn_scale"), (bn_shift, "bn_shift")):
        _chk(t, nm, torch.float32, 1)
    _chk(nbr, "nbr", torch.int32, 2)
    _chk(row_order, "row_order", torch.int32, 1)
    _chk(res, "res", x.dtype, 2)
    _chk(res_index, "res_index", torch.int32, 1)
    _chk(plan, "plan", torch.uint8, 1)
    m, c = nbr.shape[0], x.shape[1]
    if nbr.shape[1] != 27 or x.shape[0] != m:
        raise RuntimeError("conv_halo: x must have one row per row of the 27-tap neighbour table")
    if w.numel() != c * 27 * c:
        raise RuntimeError(f"conv_halo: weight has {w.numel()} elements, expected {c}x27x{c}")
    for t in (bias, bn_scale, bn_shift):
        if t is not None and t.numel() != c:
            raise RuntimeError("conv_halo: epilogue vector length != c")
    if res is not None:
        if res.shape[1] != c or (res_index is None and res.shape[0] != m):
            raise RuntimeError("conv_halo: residual shape mismatch")
        if res_index is not None and res_index.shape[0] != m:
            raise RuntimeError("conv_halo: res_index length != m")
    if row_order is not None and row_order.shape[0] != m:
        raise RuntimeError("conv_halo: row_order length != m")
    if out is None:
        out = torch.empty((m, c), dtype=x.dtype, device=x.device)
    _chk(out, "out", x.dtype, 2)
    if tuple(out.shape) != (m, c):
        raise RuntimeError("conv_halo: out shape mismatch")
    out2 = torch.empty_like(out) if dual else None
    lib.check(lib.ptv3_conv_halo(_p(x), _p(w), _p(out), m, c, _p(nbr), _p(row_order), _p(plan), plan.numel(), _p(bias),
                                 _p(bn_scale), _p(bn_shift), int(act), _p(res), _p(res_index), _p(out2), _dt(x),
                                 _stream()), "ptv3_conv_halo")
    return (out, out2) if dual else out


def conv_head_halo_policy(m, c, dtype):
    """Whether the executor runs the 3^3 conv and the head of a c-channel block of m rows as one kernel
    (PTV3_CONV_HEAD, PTV3_CONV_HEAD_MIN_ROWS)."""
    return bool(lib.ptv3_conv_head_halo_policy(int(m), int(c), _DT[dtype]))


def conv_head_halo(x, w, conv_bias, nbr, plan, shortcut, g0, b0, g1, b1, wqkv, bqkv, eps, row_order=None):
    """f1, qkv of conv_halo(x, w, nbr, plan, bias=conv_bias, row_order=row_order) followed by block_head, in one launch
    (ptv3_conv_head_halo) and bitwise their result; wqkv is chain_permute'd."""
    _chk(x, "x", (torch.float32, torch.bfloat16), 2)
    _chk(w, "w", x.dtype)
    _chk(shortcut, "shortcut", x.dtype, 2)
    _chk(wqkv, "wqkv", x.dtype, 2)
    for t, nm in ((conv_bias, "conv_bias"), (g0, "g0"), (b0, "b0"), (g1, "g1"), (b1, "b1"), (bqkv, "bqkv")):
        _chk(t, nm, torch.float32, 1)
    _chk(nbr, "nbr", torch.int32, 2)
    _chk(row_order, "row_order", torch.int32, 1)
    _chk(plan, "plan", torch.uint8, 1)
    m, c = nbr.shape[0], x.shape[1]
    if nbr.shape[1] != 27 or x.shape[0] != m or tuple(shortcut.shape) != (m, c):
        raise RuntimeError("conv_head_halo: x and shortcut must have one row per row of the 27-tap neighbour table")
    if w.numel() != c * 27 * c or tuple(wqkv.shape) != (3 * c, c):
        raise RuntimeError(f"conv_head_halo: weights must be {c}x27x{c} and {3 * c}x{c}")
    for t, n in ((conv_bias, c), (g0, c), (b0, c), (g1, c), (b1, c), (bqkv, 3 * c)):
        if t is None or t.numel() != n:
            raise RuntimeError("conv_head_halo: per-channel vector missing or of the wrong length")
    if row_order is not None and row_order.shape[0] != m:
        raise RuntimeError("conv_head_halo: row_order length != m")
    f1 = torch.empty_like(shortcut)
    qkv = torch.empty((m, 3 * c), dtype=x.dtype, device=x.device)
    lib.check(lib.ptv3_conv_head_halo(_p(x), _p(w), _p(conv_bias), m, c, _p(nbr), _p(row_order), _p(plan), plan.numel(),
                                      _p(shortcut), _p(g0), _p(b0), _p(g1), _p(b1), _p(wqkv), _p(bqkv), _p(f1), _p(qkv),
                                      float(eps), _dt(x), _stream()), "ptv3_conv_head_halo")
    return f1, qkv


def gemm_splits(m, cin, cout, kvol, dtype):
    """K slabs ptv3_gemm splits the shape into (1: a single pass)."""
    return int(lib.ptv3_gemm_splits(int(m), int(cin), int(cout), int(kvol), _DT[dtype]))


def block_fusable(c, hidden, dtype, m=0):
    """0: no fused block kernels; 1: wave-local register chain (chain_permute'd weights); 2: workgroup-cooperative
    (natural weights)."""
    return int(lib.ptv3_block_fusable(int(c), int(hidden), _DT[dtype], int(m)))


def chain_permute(w, dtype):
    """Input-channel order the register-chained GEMMs of the fused block kernels expect (bf16: inside every
    32-chunk [0-3,16-19,4-7,20-23,8-11,24-27,12-15,28-31]; fp32: unchanged)."""
    if dtype == torch.float32:
        return w
    k = w.shape[1]
    assert k % 32 == 0
    base = [(4 * g + e) if e < 4 else (16 + 4 * g + e - 4) for g in range(4) for e in range(8)]
    perm = torch.tensor([32 * q + b for q in range(k // 32) for b in base], device=w.device)
    return w.index_select(1, perm).contiguous()


def conv_slabs(x, w, nbr, kvol, row_order=None):
    """Sparse conv left as split-K fp32 slabs (no bias): (slab tensor, splits) or None when the shape does not split."""
    m, cin, cout = nbr.shape[0], x.shape[1], w.shape[0]
    dt = _dt(x)
    splits = lib.ptv3_gemm_splits(m, cin, cout, int(kvol), dt)
    if splits <= 1:
        return None
    ws_bytes = lib.ptv3_gemm_workspace_bytes(m, cin, cout, int(kvol), dt)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device)
    lib.check(lib.ptv3_gemm(_p(x), _p(w), None, m, cin, cout, int(kvol), _p(nbr), _p(row_order), None, None, None, 0,
                            None, None, None, dt, _p(ws), ws_bytes, _stream()), "ptv3_gemm(slabs)")
    return ws, splits


def rows_linear_rows():
    """row count from which the callers prefer ptv3_rows_linear to LayerNorm + tiled GEMM launches (PTV3_ROWS_MIN)"""
    import os
    return int(os.environ.get("PTV3_ROWS_MIN", "0"))


def rows_linear_capable(c, cout, dtype, m):
    return bool(lib.ptv3_rows_linear_capable(int(c), int(cout), _DT[dtype], int(m)))


def rows_linear(x, w, bias, act=ACT_NONE, res=None, ln=None, ln0=None, shortcut=None, eps=1e-5):
    """out = act(prologue(x) @ w^T + bias) [+ res] (see ptv3_rows_linear).  ln = (gamma, beta) of the LayerNorm in front
    of the GEMM; ln0 = (gamma, beta) + `shortcut`: f1 = LayerNorm(x; ln0) + shortcut first -> returns (f1, out)."""
    _chk(x, "x", (torch.float32, torch.bfloat16), 2)
    _chk(w, "w", x.dtype, 2)
    m, c = x.shape
    cout = w.shape[0]
    out = torch.empty((m, cout), dtype=x.dtype, device=x.device)
    f1 = torch.empty_like(x) if ln0 is not None else None
    g0, b0 = ln0 if ln0 is not None else (None, None)
    g1, b1 = ln if ln is not None else (None, None)
    lib.check(lib.ptv3_rows_linear(_p(x), _p(shortcut), _p(g0), _p(b0), _p(g1), _p(b1), _p(w), _p(bias), int(act), _p(res),
                                   _p(f1), _p(out), m, c, cout, float(eps), _dt(x), _stream()), "ptv3_rows_linear")
    return (f1, out) if ln0 is not None else out


def rows_linear_ln_capable(c, cout, dtype):
    return dtype in _DT and bool(lib.ptv3_rows_linear_ln_capable(int(c), int(cout), _DT[dtype]))


def subm_conv_ln_capable(c, kvol, dtype):
    return dtype in _DT and bool(lib.ptv3_subm_conv_ln_capable(int(c), int(kvol), _DT[dtype]))


def _chk_ln(name, cout, bias, gamma, beta):
    for t, nm in ((bias, "bias"), (gamma, "gamma"), (beta, "beta")):
        _chk(t, f"{name}: {nm}", torch.float32, 1)
        if t is not None and t.numel() != cout:
            raise RuntimeError(f"{name}: {nm} has {t.numel()} entries, expected {cout}")


def rows_linear_ln(x, w, bias, gamma, beta, eps=1e-5, act=ACT_RELU, out=None):
    """act(LayerNorm(x @ w^T [+ bias]; gamma, beta)) in one launch (see ptv3_rows_linear_ln): x (m, c), w (cout, c)."""
    _chk(x, "x", (torch.float32, torch.bfloat16), 2)
    _chk(w, "w", x.dtype, 2)
    m, c = x.shape
    cout = w.shape[0]
    if w.shape[1] != c:
        raise RuntimeError(f"rows_linear_ln: weight {tuple(w.shape)} does not match x {tuple(x.shape)}")
    _chk_ln("rows_linear_ln", cout, bias, gamma, beta)
    if out is None:
        out = torch.empty((m, cout), dtype=x.dtype, device=x.device)
    _chk(out, "out", x.dtype, 2)
    if tuple(out.shape) != (m, cout):
        raise RuntimeError("rows_linear_ln: out shape mismatch")
    lib.check(lib.ptv3_rows_linear_ln(_p(x), _p(w), _p(bias), _p(gamma), _p(beta), _p(out), m, c, cout, float(eps),
                                      int(act), _dt(x), _stream()), "ptv3_rows_linear_ln")
    return out


def subm_conv_ln(x, w, nbr, bias, gamma, beta, eps=1e-5, act=ACT_RELU, row_order=None, out=None):
    """act(LayerNorm(sum_t w[:, t, :] x[nbr[i][t]] [+ bias]; gamma, beta)) in one launch (see ptv3_subm_conv_ln):
    x (m, c), w (c, kvol, c) or (c, kvol * c), nbr (m, kvol) int32 with -1 for absent taps."""
    _chk(x, "x", (torch.float32, torch.bfloat16), 2)
    _chk(w, "w", x.dtype)
    _chk(nbr, "nbr", torch.int32, 2)
    _chk(row_order, "row_order", torch.int32, 1)
    m, c = x.shape
    kvol = nbr.shape[1]
    if nbr.shape[0] != m:
        raise RuntimeError("subm_conv_ln: neighbour table has another row count than x")
    if w.numel() != c * kvol * c:
        raise RuntimeError(f"subm_conv_ln: weight has {w.numel()} elements, expected {c}x{kvol}x{c}")
    if row_order is not None and row_order.shape[0] != m:
        raise RuntimeError("subm_conv_ln: row_order length != m")
    _chk_ln("subm_conv_ln", c, bias, gamma, beta)
    if out is None:
        out = torch.empty((m, c), dtype=x.dtype, device=x.device)
    _chk(out, "out", x.dtype, 2)
    if tuple(out.shape) != (m, c):
        raise RuntimeError("subm_conv_ln: out shape mismatch")
    lib.check(lib.ptv3_subm_conv_ln(_p(x), _p(w), _p(nbr), _p(row_order), _p(bias), _p(gamma), _p(beta), _p(out), m, c,
                                    int(kvol), float(eps), int(act), _dt(x), _stream()), "ptv3_subm_conv_ln")
    return out


def block_head(x, slab, splits, conv_bias, shortcut, g0, b0, g1, b1, wqkv, bqkv, eps):
    """f1, qkv of the fused head (see ptv3_block_head)."""
    _chk(shortcut, "shortcut", (torch.float32, torch.bfloat16), 2)
    m, c = shortcut.shape
    f1 = torch.empty_like(shortcut)
    qkv = torch.empty((m, 3 * c), dtype=shortcut.dtype, device=shortcut.device)
    lib.check(lib.ptv3_block_head(_p(x), _p(slab), int(splits), _p(conv_bias), _p(shortcut), _p(g0), _p(b0), _p(g1),
                                  _p(b1), _p(wqkv), _p(bqkv), _p(f1), _p(qkv), m, c, float(eps), _dt(shortcut),
                                  _stream()), "ptv3_block_head")
    return f1, qkv


def block_tail(attn, f1, wproj, bproj, g2, b2, w1, bias1, w2, bias2, eps):
    _chk(attn, "attn", (torch.float32, torch.bfloat16), 2)
    _chk(f1, "f1", attn.dtype, 2)
    m, c = attn.shape
    out = torch.empty_like(attn)
    lib.check(lib.ptv3_block_tail(_p(attn), _p(f1), _p(wproj), _p(bproj), _p(g2), _p(b2), _p(w1), _p(bias1), _p(w2),
                                  _p(bias2), _p(out), m, c, int(w1.shape[0]), float(eps), _dt(attn), _stream()),
              "ptv3_block_tail")
    return out


def block_tail_sliced_policy(c, hidden, dtype, m):
    """group count with which the executor takes ptv3_block_tail_sliced for a block of m rows, 0 where it does not
    (PTV3_TAIL_SLICED, PTV3_TAIL_SLICED_GROUPS)."""
    return int(lib.ptv3_block_tail_sliced_policy(int(c), int(hidden), _DT[dtype], int(m)))


def block_tail_sliced(attn, f1, wproj, bproj, g2, b2, w1, bias1, w2, bias2, eps, groups=0, out=None, workspace=None):
    """ops.block_tail for few rows at c = 128 or 256 in bf16 (ptv3_block_tail_sliced): the hidden layer cut across `groups`
    workgroups per row tile, fp32 partials in `workspace`, summed in group order.  Weights in natural layout."""
    _chk(attn, "attn", (torch.float32, torch.bfloat16), 2)
    _chk(f1, "f1", attn.dtype, 2)
    m, c = attn.shape
    if tuple(f1.shape) != (m, c):
        raise RuntimeError("block_tail_sliced: attn and f1 must have the same shape")
    hidden = int(w1.shape[0])
    if tuple(wproj.shape) != (c, c) or tuple(w1.shape) != (hidden, c) or tuple(w2.shape) != (c, hidden):
        raise RuntimeError(f"block_tail_sliced: weights must be {c}x{c}, {hidden}x{c} and {c}x{hidden}")
    for t, n in ((bproj, c), (g2, c), (b2, c), (bias1, hidden), (bias2, c)):
        _chk(t, "block_tail_sliced: per-channel vector", torch.float32, 1)
        if t is None or t.numel() != n:
            raise RuntimeError("block_tail_sliced: per-channel vector missing or of the wrong length")
    for t in (wproj, w1, w2):
        _chk(t, "block_tail_sliced: weight", attn.dtype, 2)
    if out is None:
        out = torch.empty_like(attn)
    _chk(out, "out", attn.dtype, 2)
    if tuple(out.shape) != (m, c):
        raise RuntimeError("block_tail_sliced: out shape mismatch")
    if workspace is None:
        g = int(groups) or block_tail_sliced_policy(c, hidden, attn.dtype, m)
        nbytes = lib.ptv3_block_tail_sliced_workspace_bytes(m, c, g) if attn.dtype in _DT else 0
        workspace = torch.empty(nbytes, dtype=torch.uint8, device=attn.device) if nbytes else None
    lib.check(lib.ptv3_block_tail_sliced(_p(attn), _p(f1), _p(wproj), _p(bproj), _p(g2), _p(b2), _p(w1), _p(bias1),
                                         _p(w2), _p(bias2), _p(out), m, c, hidden, float(eps), _dt(attn), int(groups),
                                         _p(workspace), 0 if workspace is None else workspace.numel() * workspace.element_size(),
                                         _stream()), "ptv3_block_tail_sliced")
    return out


def mlp2_fusable(cin, hidden, cout, dtype):
    return bool(lib.ptv3_mlp2_fusable(int(cin), int(hidden), int(cout), _DT[dtype]))


def mlp2_weight2(w2, dtype):
    """(cout, hidden) parameter -> the (16 | 32 | 64, hidden) chain-permuted matrix ptv3_mlp2 reads (rows beyond
    cout are zero; the kernel works on 1, 2 or 4 output tiles)."""
    w = w2.detach().to(dtype)
    rows = 16 if w.shape[0] <= 16 else 32 if w.shape[0] <= 32 else 64
    pad = rows - w.shape[0]
    if pad:
        w = torch.nn.functional.pad(w, (0, 0, 0, pad))
    return chain_permute(w.contiguous(), dtype)


def mlp2(x, w1, b1, s1, t1, act, w2p, b2, cout, out_f32=True):
    """act((x w1^T + b1) * s1 + t1) w2^T + b2 with the hidden layer in registers; w2p from mlp2_weight2."""
    _chk(x, "x", (torch.float32, torch.bfloat16), 2)
    _chk(w1, "w1", x.dtype, 2)
    _chk(w2p, "w2p", x.dtype, 2)
    for t, nm in ((b1, "b1"), (s1, "s1"), (t1, "t1"), (b2, "b2")):
        _chk(t, nm, torch.float32, 1)
    m, cin = x.shape
    hidden = w1.shape[0]
    if w1.shape[1] != cin or w2p.shape[1] != hidden or w2p.shape[0] < cout or w2p.shape[0] % 16:
        raise RuntimeError("mlp2: shape mismatch")
    out = torch.empty((m, cout), dtype=torch.float32 if out_f32 else x.dtype, device=x.device)
    lib.check(lib.ptv3_mlp2(_p(x), _p(w1), _p(b1), _p(s1), _p(t1), int(act), _p(w2p), _p(b2), _p(out), int(out_f32), m,
                            cin, hidden, int(cout), _dt(x), _stream()), "ptv3_mlp2")
    return out


def layernorm(x, gamma, beta, eps=1e-5, res=None, gamma2=None, beta2=None):
    """y = LN(x)*g+b (+res); with gamma2/beta2 also returns y2 = LN(y)*g2+b2."""
    _chk(x, "x", (torch.float32, torch.bfloat16), 2)
    _chk(gamma, "gamma", torch.float32, 1)
    _chk(beta, "beta", torch.float32, 1)
    _chk(res, "res", x.dtype, 2)
    _chk(gamma2, "gamma2", torch.float32, 1)
    _chk(beta2, "beta2", torch.float32, 1)
    m, c = x.shape
    if gamma.numel() != c or beta.numel() != c or (res is not None and res.shape != x.shape):
        raise RuntimeError("layernorm: shape mismatch")
    y = torch.empty_like(x)
    y2 = torch.empty_like(x) if gamma2 is not None else None
    lib.check(lib.ptv3_layernorm(_p(x), _p(gamma), _p(beta), _p(res), _p(y), _p(gamma2), _p(beta2), _p(y2), m, c,
                                 float(eps), _dt(x), _stream()), "ptv3_layernorm")
    return (y, y2) if gamma2 is not None else y


def layernorm_slabs(slab, splits, m, c, slab_bias, dtype, gamma, beta, eps=1e-5, res=None, gamma2=None, beta2=None):
    """layernorm() whose input is still the split-K slabs of conv_slabs() (its workspace tensor, `splits` slabs of
    (m, c) fp32): x = dtype(sum slabs + slab_bias)."""
    _chk(slab, "slab", (torch.uint8, torch.float32))
    _chk(slab_bias, "slab_bias", torch.float32, 1)
    _chk(res, "res", dtype, 2)
    if slab.numel() * slab.element_size() < splits * m * c * 4:
        raise RuntimeError("layernorm_slabs: slab buffer too small")
    y = torch.empty((m, c), dtype=dtype, device=slab.device)
    y2 = torch.empty_like(y) if gamma2 is not None else None
    lib.check(lib.ptv3_layernorm_slabs(_p(slab), int(splits), _p(slab_bias), _p(gamma), _p(beta), _p(res), _p(y),
                                       _p(gamma2), _p(beta2), _p(y2), m, c, float(eps), _DT[dtype], _stream()),
              "ptv3_layernorm_slabs")
    return (y, y2) if gamma2 is not None else y


def affine_act(x, scale, shift, act):
    _chk(x, "x", (torch.float32, torch.bfloat16), 2)
    _chk(scale, "scale", torch.float32, 1)
    _chk(shift, "shift", torch.float32, 1)
    m, c = x.shape
    y = torch.empty_like(x)
    lib.check(lib.ptv3_affine_act(_p(x), _p(scale), _p(shift), int(act), _p(y), m, c, _dt(x), _stream()),
              "ptv3_affine_act")
    return y


def cast(x, dtype):
    if x.dtype == dtype:
        return x
    _chk(x, "x", (torch.float32, torch.bfloat16))
    y = torch.empty(x.shape, dtype=dtype, device=x.device)
    lib.check(lib.ptv3_cast(_p(x), _dt(x), _p(y), _DT[dtype], x.numel(), _stream()), "ptv3_cast")
    return y


# ---------------------------------------------------------------------------------------------
# serialized pooling
# ---------------------------------------------------------------------------------------------
def pool_segments(code0, order0, shift_bits, batch=None, num_scenes=0):
    """cluster (n) int64, seg_start (n_out+1) int32, n_out (python int; ONE host sync, as torch.unique).
    With batch: also the pooled Point's cumulative offsets, returned as (device tensor, host list); a scene
    without points repeats its predecessor's offset (0 for a leading one)."""
    _chk(code0, "code0", torch.int64, 1)
    _chk(order0, "order0", torch.int64, 1)
    _chk(batch, "batch", torch.int64, 1)
    n = code0.shape[0]
    # the kernel writes a scene's entry from that scene's last point, so a scene without points keeps the -1
    pooled_offset = torch.full((num_scenes,), -1, dtype=torch.int64, device=code0.device) if batch is not None else None
    cluster = torch.empty(n, dtype=torch.int64, device=code0.device)
    seg_start = torch.empty(n + 1, dtype=torch.int32, device=code0.device)
    n_out = torch.empty(1, dtype=torch.int32, device=code0.device)
    ws_bytes = lib.ptv3_pool_workspace_bytes(n)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=code0.device)
    lib.check(lib.ptv3_pool_segments(_p(code0), _p(order0), n, int(shift_bits), _p(batch), _p(cluster),
                                     _p(seg_start), _p(n_out), _p(pooled_offset), _p(ws), ws_bytes, _stream()),
              "ptv3_pool_segments")
    if batch is not None:
        host = [int(v) for v in pooled_offset.tolist()]  # the one sync; n_out is the last entry
        if min(host) < 0:  # empty scenes (rare): forward-fill on the host, then rewrite the device copy
            for b, v in enumerate(host):
                if v < 0:
                    host[b] = host[b - 1] if b else 0
            pooled_offset.copy_(torch.tensor(host, dtype=torch.int64))
        return cluster, seg_start[:host[-1] + 1], host[-1], pooled_offset, host
    cnt = int(n_out.item())
    return cluster, seg_start[:cnt + 1], cnt


def pool_reduce(feat, coord, grid_coord, batch, code, order0, seg_start, n_out, pooling_depth, bn_scale=None,
                bn_shift=None, act=ACT_NONE, row_perm=None):
    _chk(feat, "feat", (torch.float32, torch.bfloat16), 2)
    _chk(coord, "coord", torch.float32, 2)
    _chk(grid_coord, "grid_coord", torch.int64, 2)
    _chk(batch, "batch", torch.int64, 1)
    _chk(code, "code", torch.int64, 2)
    _chk(order0, "order0", torch.int64, 1)
    _chk(seg_start, "seg_start", torch.int32, 1)
    n, c = feat.shape
    k = code.shape[0]
    dev = feat.device
    feat_out = torch.empty((n_out, c), dtype=feat.dtype, device=dev)
    coord_out = torch.empty((n_out, 3), dtype=torch.float32, device=dev) if coord is not None else None
    grid_out = torch.empty((n_out, 3), dtype=torch.int64, device=dev)
    batch_out = torch.empty(n_out, dtype=torch.int64, device=dev)
    code_out = torch.empty((k, n_out), dtype=torch.int64, device=dev)
    lib.check(lib.ptv3_pool_reduce(_p(feat), _p(coord), _p(grid_coord), _p(batch), _p(code), k, _p(order0),
                                   _p(seg_start), n, n_out, c, int(pooling_depth), _p(bn_scale), _p(bn_shift),
                                   int(act), (ctypes.c_int * k)(*row_perm) if row_perm is not None else None,
                                   _p(feat_out), _p(coord_out), _p(grid_out), _p(batch_out), _p(code_out),
                                   _dt(feat), _stream()), "ptv3_pool_reduce")
    return feat_out, coord_out, grid_out, batch_out, code_out


def pool_geometry(coord, grid_coord, batch, code, order0, seg_start, n_out, pooling_depth, row_perm=None):
    """The geometry half of ptv3_pool_reduce alone (no feature matrix): coord mean, grid >> depth, batch and the
    pooled codes of every cluster - what a training forward can compute for ALL pooling stages before the first
    feature kernel (the host syncs of pool_segments then fall on a near-empty queue)."""
    _chk(coord, "coord", torch.float32, 2)
    _chk(grid_coord, "grid_coord", torch.int64, 2)
    _chk(batch, "batch", torch.int64, 1)
    _chk(code, "code", torch.int64, 2)
    _chk(order0, "order0", torch.int64, 1)
    _chk(seg_start, "seg_start", torch.int32, 1)
    k, n = code.shape
    dev = code.device
    coord_out = torch.empty((n_out, 3), dtype=torch.float32, device=dev) if coord is not None else None
    grid_out = torch.empty((n_out, 3), dtype=torch.int64, device=dev)
    batch_out = torch.empty(n_out, dtype=torch.int64, device=dev)
    code_out = torch.empty((k, n_out), dtype=torch.int64, device=dev)
    lib.check(lib.ptv3_pool_reduce(None, _p(coord), _p(grid_coord), _p(batch), _p(code), k, _p(order0), _p(seg_start), n,
                                   n_out, 4, int(pooling_depth), None, None, ACT_NONE,
                                   (ctypes.c_int * k)(*row_perm) if row_perm is not None else None, None, _p(coord_out),
                                   _p(grid_out), _p(batch_out), _p(code_out), PTV3_F32, _stream()), "ptv3_pool_reduce")
    return coord_out, grid_out, batch_out, code_out


# ---------------------------------------------------------------------------------------------
# training: backward kernels
# ---------------------------------------------------------------------------------------------
_F = (torch.float32, torch.bfloat16)


def _ws(nbytes, dev):
    return torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=dev)


def gemm_tn(dy, x, nbr=None, kvol=1, with_bias=False):
    """dW (cout, kvol*cin) fp32 = dy^T . gather(x): weight gradient of a Linear (kvol=1) or SubMConv3d.
    with_bias: -> (dW, db) with db (cout) fp32 = column sums of dy from the same pass."""
    _chk(dy, "dy", _F, 2)
    _chk(x, "x", dy.dtype, 2)
    _chk(nbr, "nbr", torch.int32, 2)
    m, cout = dy.shape
    cin = x.shape[1]
    if (nbr is None) != (kvol == 1) or (nbr is not None and tuple(nbr.shape) != (m, kvol)) or \
            (nbr is None and x.shape[0] != m):
        raise RuntimeError("gemm_tn: shape mismatch")
    dw = torch.empty((cout, kvol * cin), dtype=torch.float32, device=dy.device)
    db = torch.empty(cout, dtype=torch.float32, device=dy.device) if with_bias else None
    nb = lib.ptv3_gemm_tn_workspace_bytes(m, cout, cin, int(kvol))
    ws = _ws(nb, dy.device)
    lib.check(lib.ptv3_gemm_tn(_p(dy), _p(x), _p(nbr), _p(dw), _p(db), m, cout, cin, int(kvol), _dt(dy), _p(ws), nb,
                               _stream()), "ptv3_gemm_tn")
    return (dw, db) if with_bias else dw


def col_reduce(a, b=None, mu=None, rs=None, mode=0, mu_scale=1.0):
    """fp32 column sums over rows: mode 0 (c) sum a; 1 (2, c) sum a, sum a^2; 2 (2, c) sum a, sum a*(b-mu)*rs;
    3 (2, c) sum a, sum (a-mu)^2.  mu is multiplied by mu_scale (column sums and 1 / m instead of a mean tensor)."""
    _chk(a, "a", _F, 2)
    _chk(b, "b", a.dtype, 2)
    _chk(mu, "mu", torch.float32, 1)
    _chk(rs, "rs", torch.float32, 1)
    m, c = a.shape
    out = torch.empty((1 if mode == 0 else 2, c), dtype=torch.float32, device=a.device)
    nb = lib.ptv3_col_reduce_workspace_bytes(m, c)
    ws = _ws(nb, a.device)
    lib.check(lib.ptv3_col_reduce(_p(a), _p(b), _p(mu), _p(rs), float(mu_scale), int(mode), _p(out), m, c, _dt(a), _p(ws),
                                  nb, _stream()), "ptv3_col_reduce")
    return out[0] if mode == 0 else out


def bn_finalize(total, centred_sq, m, weight, bias, running_mean, running_var, momentum, eps):
    """-> mean, rstd, scale, shift (c) fp32 of a BatchNorm1d training forward; running buffers updated in place."""
    for t, nm in ((total, "total"), (centred_sq, "centred_sq"), (weight, "weight"), (bias, "bias"),
                  (running_mean, "running_mean"), (running_var, "running_var")):
        _chk(t, nm, torch.float32, 1)
    c = total.shape[0]
    out = torch.empty((4, c), dtype=torch.float32, device=total.device)
    lib.check(lib.ptv3_bn_finalize(_p(total), _p(centred_sq), int(m), _p(weight), _p(bias), _p(running_mean),
                                   _p(running_var), float(momentum), float(eps), _p(out[0]), _p(out[1]), _p(out[2]),
                                   _p(out[3]), c, _stream()), "ptv3_bn_finalize")
    return out[0], out[1], out[2], out[3]


def bn_bwd_coeffs(sums, m, weight, rstd, mean):
    """-> ca, cb, cc (c) fp32: BatchNorm1d input gradient dx = ca dy + cb x + cc from the two batch sums of mode 2."""
    _chk(sums, "sums", torch.float32, 2)
    c = sums.shape[1]
    out = torch.empty((3, c), dtype=torch.float32, device=sums.device)
    lib.check(lib.ptv3_bn_bwd_coeffs(_p(sums), int(m), _p(weight), _p(rstd), _p(mean), _p(out[0]), _p(out[1]), _p(out[2]),
                                     c, _stream()), "ptv3_bn_bwd_coeffs")
    return out[0], out[1], out[2]


def layernorm_bwd(x, dy, gamma, eps, add=None):
    """-> dx (m, c) [+ add], dgamma (c), dbeta (c)."""
    _chk(x, "x", _F, 2)
    _chk(dy, "dy", x.dtype, 2)
    _chk(add, "add", x.dtype, 2)
    if add is not None and add.shape != x.shape:
        raise RuntimeError("layernorm_bwd: add must have the shape of x")
    _chk(gamma, "gamma", torch.float32, 1)
    m, c = x.shape
    dx = torch.empty_like(x)
    dgb = torch.empty((2, c), dtype=torch.float32, device=x.device)
    nb = lib.ptv3_col_reduce_workspace_bytes(m, c)
    ws = _ws(nb, x.device)
    lib.check(lib.ptv3_layernorm_bwd(_p(x), _p(dy), _p(add), _p(gamma), float(eps), _p(dx), _p(dgb), m, c, _dt(x), _p(ws), nb,
                                     _stream()), "ptv3_layernorm_bwd")
    return dx, dgb[0], dgb[1]


def act_bwd(dy, x, act, scale=None, shift=None):
    """dy * act'(x*scale + shift)."""
    _chk(dy, "dy", _F, 2)
    _chk(x, "x", dy.dtype, 2)
    _chk(scale, "scale", torch.float32, 1)
    _chk(shift, "shift", torch.float32, 1)
    m, c = x.shape
    dx = torch.empty_like(x)
    lib.check(lib.ptv3_act_bwd(_p(dy), _p(x), _p(scale), _p(shift), int(act), _p(dx), m, c, _dt(x), _stream()),
              "ptv3_act_bwd")
    return dx


def affine2(dy, x, ca, cb, cc):
    """ca*dy + cb*x + cc per column."""
    _chk(dy, "dy", _F, 2)
    _chk(x, "x", dy.dtype, 2)
    for t, nm in ((ca, "ca"), (cb, "cb"), (cc, "cc")):
        _chk(t, nm, torch.float32, 1)
    m, c = x.shape
    dx = torch.empty_like(x)
    lib.check(lib.ptv3_affine2(_p(dy), _p(x), _p(ca), _p(cb), _p(cc), _p(dx), m, c, _dt(x), _stream()), "ptv3_affine2")
    return dx


def pool_max(feat, order0, seg_start, n_out):
    """segment max over the members of each cluster (the feature half of ptv3_pool_reduce, no BN / act)."""
    _chk(feat, "feat", _F, 2)
    _chk(order0, "order0", torch.int64, 1)
    _chk(seg_start, "seg_start", torch.int32, 1)
    n, c = feat.shape
    out = torch.empty((n_out, c), dtype=feat.dtype, device=feat.device)
    lib.check(lib.ptv3_pool_reduce(_p(feat), None, None, None, None, 1, _p(order0), _p(seg_start), n, n_out, c, 0, None,
                                   None, ACT_NONE, None, _p(out), None, None, None, None, _dt(feat), _stream()),
              "ptv3_pool_reduce")
    return out


def pool_max_bwd(feat, dy, order0, seg_start):
    _chk(feat, "feat", _F, 2)
    _chk(dy, "dy", feat.dtype, 2)
    n_out, c = dy.shape
    dfeat = torch.empty_like(feat)
    lib.check(lib.ptv3_pool_max_bwd(_p(feat), _p(dy), _p(order0), _p(seg_start), n_out, c, _p(dfeat), _dt(feat),
                                    _stream()), "ptv3_pool_max_bwd")
    return dfeat


def segment_sum(dy, order0, seg_start, n_out):
    _chk(dy, "dy", _F, 2)
    c = dy.shape[1]
    out = torch.empty((n_out, c), dtype=dy.dtype, device=dy.device)
    lib.check(lib.ptv3_segment_sum(_p(dy), _p(order0), _p(seg_start), n_out, c, _p(out), _dt(dy), _stream()),
              "ptv3_segment_sum")
    return out


def window_attention_bwd(qkv, out, dout, win_order, win_inverse, heads, patch, scale, cu_seqlens=None):
    n, c, n_pad, nwin = _attn_check("window_attention_bwd", qkv, win_order, win_inverse, heads, patch, cu_seqlens, out, dout)
    dqkv = torch.empty_like(qkv)
    nb = lib.ptv3_window_attn_bwd_workspace_bytes(n, n_pad, c, int(heads), _dt(qkv))
    ws = _ws(nb, qkv.device)
    if cu_seqlens is not None:
        lib.check(lib.ptv3_window_attn_varlen_bwd(_p(qkv), _p(out), _p(dout), _p(win_order), _p(win_inverse),
                                                  _p(cu_seqlens), nwin, _p(dqkv), n, n_pad, c, int(heads), int(patch),
                                                  float(scale), _dt(qkv), _p(ws), nb, _stream()),
                  "ptv3_window_attn_varlen_bwd")
        return dqkv
    lib.check(lib.ptv3_window_attn_bwd(_p(qkv), _p(out), _p(dout), _p(win_order), _p(win_inverse), _p(dqkv), n, n_pad,
                                       c, int(heads), int(patch), float(scale), _dt(qkv), _p(ws), nb, _stream()),
              "ptv3_window_attn_bwd")
    return dqkv


def window_attention_rpe_bwd(qkv, out, dout, win_order, win_inverse, heads, patch, scale, grid_coord, rpe_table,
                             pos_bnd):
    """-> (dqkv (n, 3c), dtable (3*(2*pos_bnd+1), heads) fp32) of window_attention_rpe."""
    n, c, n_pad, _ = _attn_check("window_attention_rpe_bwd", qkv, win_order, win_inverse, heads, patch, None, out, dout,
                                 grid_coord=grid_coord, rpe_table=rpe_table, pos_bnd=pos_bnd)
    dqkv = torch.empty_like(qkv)
    dtable = torch.empty_like(rpe_table)
    nb = lib.ptv3_window_attn_rpe_bwd_workspace_bytes(n, n_pad, c, int(heads), int(patch), int(pos_bnd), _dt(qkv))
    ws = _ws(nb, qkv.device)
    lib.check(lib.ptv3_window_attn_rpe_bwd(_p(qkv), _p(out), _p(dout), _p(win_order), _p(win_inverse), _p(grid_coord),
                                           _p(rpe_table), int(pos_bnd), _p(dqkv), _p(dtable), n, n_pad, c, int(heads),
                                           int(patch), float(scale), _dt(qkv), _p(ws), nb, _stream()),
              "ptv3_window_attn_rpe_bwd")
    return dqkv, dtable


# ---------------------------------------------------------------------------------------------
# GridSample (before the model)
# ---------------------------------------------------------------------------------------------
def grid_hash(coord, grid_size, hash_type=HASH_FNV):
    """-> grid_coord (n,3) int64 (minimum subtracted), min_max (6) int64, key (n) int64 holding the uint64 hash."""
    _chk(coord, "coord", torch.float32, 2)
    n = coord.shape[0]
    grid = torch.empty((n, 3), dtype=torch.int64, device=coord.device)
    mm = torch.empty(6, dtype=torch.int64, device=coord.device)
    key = torch.empty(n, dtype=torch.int64, device=coord.device)
    lib.check(lib.ptv3_grid_hash(_p(coord), n, float(grid_size), int(hash_type), _p(grid), _p(mm), _p(key), _stream()),
              "ptv3_grid_hash")
    return grid, mm, key


def voxel_unique(key):
    """np.argsort + np.unique(return_inverse, return_counts) of the voxel keys on the device:
    idx_sort (n) int64 (stable), inverse (n) int64 in ORIGINAL point order, seg_start (nvox+1) int32, nvox."""
    _chk(key, "key", torch.int64, 1)
    order, _ = argsort_codes(key.view(1, -1), 64)
    order = order[0].contiguous()
    cluster, seg_start, nvox = pool_segments(key, order, 0)
    return order, cluster, seg_start, nvox


# ---------------------------------------------------------------------------------------------
# Swin3D window partition + cRSE attention (row A19, parity unpinned: see oracle/swin3d.py)
# ---------------------------------------------------------------------------------------------
def swin_window_mapping(coords, stride, window_size, shift=0):
    """BasicLayer.get_window_mapping (swin3d_layers.py:746-795) of voxels `coords` (n,4) int32 [batch,x,y,z] at tensor
    stride `stride`, shifted by `shift` voxels (:826-840).  -> w_w_id (n) int64 and w_w_xyz (n,3) int64 in sorted
    order, w_sizes (W) int64, sort_idx (n) int64, inv_sort_idx (n) int64, w_start (W+1) int32.  One host sync (W)."""
    _chk(coords, "coords", torch.int32, 2)
    n = coords.shape[0]
    key = torch.empty(n, dtype=torch.int64, device=coords.device)
    bad = torch.empty(1, dtype=torch.int32, device=coords.device)
    lib.check(lib.ptv3_swin_window_keys(_p(coords), n, int(stride), int(window_size), int(shift), _p(key), _p(bad),
                                        _stream()), "ptv3_swin_window_keys")
    order, inverse = argsort_codes(key.view(1, -1), 61)
    order, inverse = order[0].contiguous(), inverse[0].contiguous()
    _, w_start, nwin = pool_segments(key, order, 9)
    if int(bad.item()):
        raise ValueError("swin_window_mapping: batch index outside 0..4095 or window coordinate outside -4096..4095")
    w_w_id = key[order] & 511
    ws = int(window_size)
    w_w_xyz = torch.stack([w_w_id // ws // ws, w_w_id // ws % ws, w_w_id % ws], dim=-1)
    w_sizes = (w_start[1:] - w_start[:-1]).long()
    return w_w_id, w_w_xyz, w_sizes, order, inverse, w_start


def swin_attention(q, k, v, q_table, k_table, v_table, table_offsets, n2n, w_start, n_crse, max_tokens):
    """SelfAttnAIOFunction forward (swin3d_layers.py:556-569): q (pre-scaled), k, v (n, H, D) in original voxel order,
    concatenated fp32 tables with `table_offsets` elements per signal axis, n2n / w_start / n_crse as
    swin_window_mapping and WindowAttention.forward build them.  -> (n, H, D) in original order."""
    _chk(q, "q", _F, 3)
    for name, t in (("k", k), ("v", v)):
        _chk(t, name, q.dtype, 3)
        if t.shape != q.shape:
            raise ValueError(f"swin_attention: {name} {tuple(t.shape)} vs q {tuple(q.shape)}")
    for name, t in (("q_table", q_table), ("k_table", k_table), ("v_table", v_table)):
        _chk(t, name, torch.float32, 1)
    _chk(n2n, "n2n", torch.int64, 1)
    _chk(w_start, "w_start", torch.int32, 1)
    _chk(n_crse, "n_crse", torch.float32, 2)
    n, heads, hd = q.shape
    axes = len(table_offsets)
    total = int(sum(int(t) for t in table_offsets))
    if n_crse.shape != (n, axes) or n2n.shape[0] != n:
        raise ValueError(f"swin_attention: n_crse {tuple(n_crse.shape)} / n2n {tuple(n2n.shape)} for {n} voxels, {axes} axes")
    if min(q_table.numel(), k_table.numel(), v_table.numel()) < total:
        raise ValueError("swin_attention: tables are shorter than sum(table_offsets)")
    out = torch.empty_like(q)
    offs = (ctypes.c_int32 * axes)(*[int(t) for t in table_offsets])
    if _PROFILING:   # the pair count is device data: read back only while the launch is being bracketed
        lens = (w_start[1:] - w_start[:-1]).double()
        lib.ptv3_profile_hint_flops(float((lens * lens).sum().item()) * heads * (1 + 3 * axes) * 2 * hd)
    lib.check(lib.ptv3_swin_attn_fwd(_p(q), _p(k), _p(v), _p(q_table), _p(k_table), _p(v_table), offs, axes, _p(n2n),
                                     _p(w_start), w_start.shape[0] - 1, _p(n_crse), _p(out), n, heads, hd,
                                     int(max_tokens), _dt(q), _stream()), "ptv3_swin_attn_fwd")
    return out


def swin_attention_bwd(q, k, v, dout, q_table, k_table, v_table, table_offsets, n2n, w_start, n_crse, max_tokens):
    """-> dq, dk, dv (n, H, D) in the dtype of q and dq_table, dk_table, dv_table (fp32, flat like the tables)."""
    _chk(q, "q", _F, 3)
    for name, t in (("k", k), ("v", v), ("dout", dout)):
        _chk(t, name, q.dtype, 3)
        if t.shape != q.shape:
            raise ValueError(f"swin_attention_bwd: {name} {tuple(t.shape)} vs q {tuple(q.shape)}")
    for name, t in (("q_table", q_table), ("k_table", k_table), ("v_table", v_table)):
        _chk(t, name, torch.float32, 1)
    _chk(n2n, "n2n", torch.int64, 1)
    _chk(w_start, "w_start", torch.int32, 1)
    _chk(n_crse, "n_crse", torch.float32, 2)
    n, heads, hd = q.shape
    axes = len(table_offsets)
    total = int(sum(int(t) for t in table_offsets))
    if n_crse.shape != (n, axes) or n2n.shape[0] != n or min(q_table.numel(), k_table.numel(), v_table.numel()) < total:
        raise ValueError("swin_attention_bwd: shapes of n_crse / n2n / tables do not fit")
    dq, dk, dv = torch.empty_like(q), torch.empty_like(q), torch.empty_like(q)
    dtab = torch.empty((3, total), dtype=torch.float32, device=q.device)
    offs = (ctypes.c_int32 * axes)(*[int(t) for t in table_offsets])
    lib.check(lib.ptv3_swin_attn_bwd(_p(q), _p(k), _p(v), _p(dout), _p(q_table), _p(k_table), _p(v_table), offs, axes,
                                     _p(n2n), _p(w_start), w_start.shape[0] - 1, _p(n_crse), _p(dq), _p(dk), _p(dv),
                                     _p(dtab[0]), _p(dtab[1]), _p(dtab[2]), n, heads, hd, int(max_tokens), _dt(q),
                                     _stream()), "ptv3_swin_attn_bwd")
    return dq, dk, dv, dtab[0], dtab[1], dtab[2]


# ---------------------------------------------------------------------------------------------
# keypoint aggregation (after the model)
# ---------------------------------------------------------------------------------------------
def keypoint_aggregate(coord, pred, offset, mode, scale=None, centroid=None, thresh=0.5):
    """(B, K, 3) keypoints + (B, K) int32 aux per scene and keypoint; see ptv3_keypoint_aggregate."""
    _chk(coord, "coord", torch.float32, 2)
    _chk(pred, "pred", torch.float32, 3)
    _chk(offset, "offset", torch.int64, 1)
    _chk(scale, "scale", torch.float32, 1)
    _chk(centroid, "centroid", torch.float32, 2)
    n, k, four = pred.shape
    b = offset.shape[0]
    if four != 4 or coord.shape != (n, 3) or (scale is not None and scale.shape[0] != b) or \
            (centroid is not None and tuple(centroid.shape) != (b, 3)):
        raise RuntimeError("keypoint_aggregate: shape mismatch")
    kp = torch.empty((b, k, 3), dtype=torch.float32, device=coord.device)
    aux = torch.empty((b, k), dtype=torch.int32, device=coord.device)
    lib.check(lib.ptv3_keypoint_aggregate(_p(coord), _p(pred), _p(offset), b, k, _p(scale), _p(centroid), int(mode),
                                          float(thresh), _p(kp), _p(aux), _stream()), "ptv3_keypoint_aggregate")
    return kp, aux


# ---------------------------------------------------------------------------------------------
# global-regression keypoint heads
# ---------------------------------------------------------------------------------------------
def _scene_offset(offset, name):
    """int32 (tools/KeyPointPrediction_Qt.py:84) or int64 cumulative scene ends -> contiguous int64, on the device."""
    _chk(offset, name, (torch.int32, torch.int64), 1)
    return offset if offset.dtype == torch.int64 else offset.long().contiguous()


def scene_mean(feat, offset):
    """(B, C) fp32 per-scene column means of feat (N, C) fp32 / bf16 (scatter_mean; an empty scene gives zeros)."""
    _chk(feat, "feat", _F, 2)
    off = _scene_offset(offset, "offset")
    n, c = feat.shape
    b = off.shape[0]
    out = torch.empty((b, c), dtype=torch.float32, device=feat.device)
    nb = lib.ptv3_scene_mean_workspace_bytes(n, c, b)
    ws = _ws(nb, feat.device)
    lib.check(lib.ptv3_scene_mean(_p(feat), _p(off), n, c, b, _dt(feat), _p(out), _p(ws), nb, _stream()),
              "ptv3_scene_mean")
    return out


def scene_mean_head(feat, offset, w1t, b1, s1, t1, w2t, b2, w3t, b3):
    """(B, out) fp32: per-scene mean of feat, then W3 relu(W2 relu((W1 g + b1) s1 + t1) + b2) + b3 in fp32 with the
    TRANSPOSED weights w1t (C, H), w2t (H, H), w3t (H, out) - two launches (ptv3_scene_mean_head)."""
    _chk(feat, "feat", _F, 2)
    off = _scene_offset(offset, "offset")
    for t, nm in ((w1t, "w1t"), (w2t, "w2t"), (w3t, "w3t")):
        _chk(t, nm, torch.float32, 2)
    for t, nm in ((b1, "b1"), (s1, "s1"), (t1, "t1"), (b2, "b2"), (b3, "b3")):
        _chk(t, nm, torch.float32, 1)
    n, c = feat.shape
    h, o = w1t.shape[1], w3t.shape[1]
    if w1t.shape[0] != c or tuple(w2t.shape) != (h, h) or w3t.shape[0] != h or \
            any(t.shape[0] != h for t in (b1, s1, t1, b2)) or b3.shape[0] != o:
        raise RuntimeError("scene_mean_head: shape mismatch")
    b = off.shape[0]
    out = torch.empty((b, o), dtype=torch.float32, device=feat.device)
    nb = lib.ptv3_scene_mean_workspace_bytes(n, c, b)
    ws = _ws(nb, feat.device)
    lib.check(lib.ptv3_scene_mean_head(_p(feat), _p(off), n, c, b, _dt(feat), _p(w1t), _p(b1), _p(s1), _p(t1), h,
                                       _p(w2t), _p(b2), _p(w3t), _p(b3), o, _p(out), _p(ws), nb, _stream()),
              "ptv3_scene_mean_head")
    return out


def scene_mean_bwd(dg, offset, n, dtype):
    """(n, C) in `dtype`: row i = dg[scene(i)] / n_scene(i), the input gradient of scene_mean."""
    _chk(dg, "dg", torch.float32, 2)
    off = _scene_offset(offset, "offset")
    b, c = dg.shape
    if off.shape[0] != b:
        raise RuntimeError("scene_mean_bwd: dg rows != number of scenes")
    dfeat = torch.empty((n, c), dtype=dtype, device=dg.device)
    lib.check(lib.ptv3_scene_mean_bwd(_p(dg), _p(off), int(n), c, b, _p(dfeat), _DT[dtype], _stream()),
              "ptv3_scene_mean_bwd")
    return dfeat


# ---------------------------------------------------------------------------------------------
# classifier / regressor head (DefaultClassifier, PigBodyRegressor)
# ---------------------------------------------------------------------------------------------
def cls_head_capable(c, h1, h2, out):
    """True when the batch head kernels take these widths (ptv3_cls_head_capable)."""
    return bool(lib.ptv3_cls_head_capable(int(c), int(h1), int(h2), int(out)))


def _cls_target(target, b, out, dev):
    if target is None:
        return None, None
    _chk(target, "target", torch.float32)
    if target.numel() != b * out:
        raise RuntimeError(f"cls_head: target has {target.numel()} elements, expected {b} x {out}")
    return target, torch.empty(1 + out, dtype=torch.float32, device=dev)


def cls_head_eval(feat, offset, w1t, b1, s1, t1, w2t, b2, s2, t2, w3t, b3, target=None, loss_weight=1.0,
                  metric_scale=1.0):
    """(logits (B, out) fp32, stats (1 + out) or None): per-scene mean of feat (N, C) fp32 / bf16, then the head with
    folded BatchNorms in fp32 on TRANSPOSED weights w1t (C, H1), w2t (H1, H2), w3t (H2, out); with `target` (B * out)
    stats = [loss_weight * mean |logits - target|, metric_scale * column means of |logits - target|].  Two launches
    (ptv3_cls_head_eval)."""
    _chk(feat, "feat", _F, 2)
    off = _scene_offset(offset, "offset")
    for t, nm in ((w1t, "w1t"), (w2t, "w2t"), (w3t, "w3t")):
        _chk(t, nm, torch.float32, 2)
    for t, nm in ((b1, "b1"), (s1, "s1"), (t1, "t1"), (b2, "b2"), (s2, "s2"), (t2, "t2"), (b3, "b3")):
        _chk(t, nm, torch.float32, 1)
    n, c = feat.shape
    h1, h2, o = w1t.shape[1], w2t.shape[1], w3t.shape[1]
    if w1t.shape[0] != c or w2t.shape[0] != h1 or w3t.shape[0] != h2 or any(t.shape[0] != h1 for t in (b1, s1, t1)) \
            or any(t.shape[0] != h2 for t in (b2, s2, t2)) or b3.shape[0] != o:
        raise RuntimeError("cls_head_eval: shape mismatch")
    b = off.shape[0]
    target, stats = _cls_target(target, b, o, feat.device)
    logits = torch.empty((b, o), dtype=torch.float32, device=feat.device)
    nb = lib.ptv3_scene_mean_workspace_bytes(n, c, b)
    ws = _ws(nb, feat.device)
    lib.check(lib.ptv3_cls_head_eval(_p(feat), _p(off), n, c, b, _dt(feat), _p(w1t), _p(b1), _p(s1), _p(t1), h1,
                                     _p(w2t), _p(b2), _p(s2), _p(t2), h2, _p(w3t), _p(b3), o, _p(target),
                                     float(loss_weight), float(metric_scale), _p(logits), _p(stats), _p(ws), nb,
                                     _stream()), "ptv3_cls_head_eval")
    return logits, stats


def _cls_params(w1, b1, g1, be1, rm1, rv1, mom1, eps1, w2, b2, g2, be2, rm2, rv2, mom2, eps2, w3, b3):
    from .lib import ClsHeadParams
    for t, nm in ((w1, "w1"), (w2, "w2"), (w3, "w3")):
        _chk(t, nm, torch.float32, 2)
    for t, nm in ((b1, "b1"), (g1, "bn1.weight"), (be1, "bn1.bias"), (rm1, "bn1.running_mean"),
                  (rv1, "bn1.running_var"), (b2, "b2"), (g2, "bn2.weight"), (be2, "bn2.bias"),
                  (rm2, "bn2.running_mean"), (rv2, "bn2.running_var"), (b3, "b3")):
        _chk(t, nm, torch.float32, 1)
    h1, c = w1.shape
    h2, o = w2.shape[0], w3.shape[0]
    if w2.shape[1] != h1 or w3.shape[1] != h2 or any(t is not None and t.shape[0] != h1 for t in (b1, g1, be1, rm1, rv1)) \
            or any(t is not None and t.shape[0] != h2 for t in (b2, g2, be2, rm2, rv2)) or b3.shape[0] != o:
        raise RuntimeError("cls_head: parameter shape mismatch")
    p = ClsHeadParams(_p(w1), _p(b1), _p(g1), _p(be1), _p(rm1), _p(rv1), _p(w2), _p(b2), _p(g2), _p(be2), _p(rm2),
                      _p(rv2), _p(w3), _p(b3), float(mom1), float(eps1), float(mom2), float(eps2))
    return p, (c, h1, h2, o)


def cls_head_train_fwd(g, params, mask1, mask2, keep, target=None, loss_weight=1.0, metric_scale=1.0):
    """Training forward of the head on the pooled rows g (B, C) fp32, one launch (ptv3_cls_head_train_fwd).
    params: the 18 arguments of _cls_params (nn.Linear's own weights; both BatchNorms' affine, running buffers - updated
    in place -, momentum, eps).  mask1 (B, H1) / mask2 (B, H2): 0 / 1 keep-masks, applied as mask / keep.
    -> (logits (B, out), stats (1 + out) or None, save): `save` is the tape cls_head_train_bwd takes."""
    _chk(g, "g", torch.float32, 2)
    p, (c, h1, h2, o) = _cls_params(*params)
    b = g.shape[0]
    _chk(mask1, "mask1", torch.float32, 2)
    _chk(mask2, "mask2", torch.float32, 2)
    if g.shape[1] != c or tuple(mask1.shape) != (b, h1) or tuple(mask2.shape) != (b, h2):
        raise RuntimeError("cls_head_train_fwd: shape mismatch")
    target, stats = _cls_target(target, b, o, g.device)
    logits = torch.empty((b, o), dtype=torch.float32, device=g.device)
    save = torch.empty(max(lib.ptv3_cls_head_save_floats(b, h1, h2, o), 1), dtype=torch.float32, device=g.device)
    lib.check(lib.ptv3_cls_head_train_fwd(_p(g), b, c, h1, h2, o, ctypes.addressof(p), _p(mask1), _p(mask2),
                                          1.0 / float(keep), _p(target), float(loss_weight), float(metric_scale),
                                          _p(save), _p(logits), _p(stats), _stream()), "ptv3_cls_head_train_fwd")
    return logits, stats, save


def cls_head_train_bwd(g, params, save, keep, dlogits=None, dloss=None, loss_weight=1.0):
    """Backward of cls_head_train_fwd, two launches (ptv3_cls_head_train_bwd).  Either dlogits (B, out) or dloss (a
    device scalar: then dlogits = dloss * loss_weight * sign(logits - target) / (B * out), sign from the tape).
    -> (dg (B, C), [dW1, db1, dbn1.weight, dbn1.bias, dW2, db2, dbn2.weight, dbn2.bias, dW3, db3])."""
    from .lib import ClsHeadGrads
    _chk(g, "g", torch.float32, 2)
    _chk(save, "save", torch.float32, 1)
    p, (c, h1, h2, o) = _cls_params(*params)
    b = g.shape[0]
    if g.shape[1] != c or save.numel() < lib.ptv3_cls_head_save_floats(b, h1, h2, o):
        raise RuntimeError("cls_head_train_bwd: shape mismatch")
    if dlogits is not None:
        _chk(dlogits, "dlogits", torch.float32, 2)
        if tuple(dlogits.shape) != (b, o):
            raise RuntimeError("cls_head_train_bwd: dlogits shape mismatch")
    if dloss is not None:
        _chk(dloss, "dloss", torch.float32)
        if dloss.numel() < 1:
            raise RuntimeError("cls_head_train_bwd: dloss is empty")
    new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=g.device)  # noqa: E731
    grads = [new(h1, c), new(h1), new(h1), new(h1), new(h2, h1), new(h2), new(h2), new(h2), new(o, h2), new(o)]
    dg = new(b, c)
    dz = new(b * (h1 + h2 + o))
    gs = ClsHeadGrads(*[_p(t) for t in grads])
    lib.check(lib.ptv3_cls_head_train_bwd(_p(g), b, c, h1, h2, o, ctypes.addressof(p), _p(dlogits), _p(dloss),
                                          float(loss_weight), 1.0 / float(keep), _p(save), _p(dz), _p(dg),
                                          ctypes.addressof(gs), _stream()), "ptv3_cls_head_train_bwd")
    return dg, grads


# ---------------------------------------------------------------------------------------------
# voting keypoint head
# ---------------------------------------------------------------------------------------------
def scene_median(x, coord, offset):
    """(B, C) fp32: the lower median over each scene's rows of x (N, C) fp32 (+ coord[:, j % 3] when coord (N, 3) is
    given) - torch.median(dim=0).values per scene (keypoint_swin3d_plus.py:166-189): NaN in a column gives NaN there, an
    empty scene zeros.  An exact selection, bitwise reproducible; B = len(offset), nothing is read back."""
    _chk(x, "x", torch.float32, 2)
    _chk(coord, "coord", torch.float32, 2)
    off = _scene_offset(offset, "offset")
    n, c = x.shape
    if coord is not None and tuple(coord.shape) != (n, 3):
        raise RuntimeError(f"scene_median: coord {tuple(coord.shape)}, expected ({n}, 3)")
    b = off.shape[0]
    out = torch.empty((b, c), dtype=torch.float32, device=x.device)
    nb = lib.ptv3_scene_median_workspace_bytes(c, b)
    ws = _ws(nb, x.device)
    lib.check(lib.ptv3_scene_median(_p(x), _p(coord), _p(off), n, c, b, _p(out), _p(ws), nb, _stream()),
              "ptv3_scene_median")
    return out


def _vote_target(target, n, k, b):
    """The reference's target layouts (keypoint_swin3d_plus.py:95-102), decided from host shapes: B * K * 3 numbers are
    per-scene rows, N leading rows are per-point rows; anything else is its ValueError.  -> (target (rows, 3), flag)"""
    if target.numel() == b * k * 3:
        return target.reshape(b * k, 3), 0
    if target.shape[0] == n and target.numel() == n * k * 3:
        return target.reshape(n * k, 3), 1
    raise ValueError("Target shape mismatch.")


def _vote_args(votes, coord, target, offset):
    _chk(votes, "votes", torch.float32, 2)
    _chk(coord, "coord", torch.float32, 2)
    _chk(target, "target", torch.float32)
    off = _scene_offset(offset, "offset")
    n = votes.shape[0]
    if votes.shape[1] % 3 or tuple(coord.shape) != (n, 3):
        raise RuntimeError(f"vote_loss: votes {tuple(votes.shape)} / coord {tuple(coord.shape)}: expected (N, 3K), (N, 3)")
    k, b = votes.shape[1] // 3, off.shape[0]
    tgt, per_point = _vote_target(target, n, k, b)
    return off, n, k, b, tgt, per_point


def vote_loss(votes, coord, target, offset, vote_radius, scale=None):
    """The vote loss and curves of keypoint_swin3d_plus.py:86-164 in two launches -> (out (2 + K) fp32 = loss,
    train/masked_dist_err, train/kp{k}_dist_err; count (1 + K) int32 = mask total, per keypoint).  votes (N, 3K) are the
    raw offsets; target (B * K, 3) / (B, K, 3) by scene or (N, K, 3) by point; scale (B) / (N), optionally (., 1)."""
    off, n, k, b, tgt, per_point = _vote_args(votes, coord, target, offset)
    scale_pp = 0
    if scale is not None:
        _chk(scale, "scale", torch.float32)
        scale_pp = int(scale.shape[0] == n)          # :127-128: anything not N long is indexed by the scene
        if scale.numel() != (n if scale_pp else b):
            raise RuntimeError(f"vote_loss: scale {tuple(scale.shape)}: expected one value per scene or per point")
    out = torch.empty(2 + k, dtype=torch.float32, device=votes.device)
    count = torch.empty(1 + k, dtype=torch.int32, device=votes.device)
    nbytes = lib.ptv3_vote_loss_workspace_bytes(n, k, b)
    ws = _ws(nbytes, votes.device)
    lib.check(lib.ptv3_vote_loss(_p(votes), _p(coord), _p(tgt), per_point, _p(off), _p(scale), scale_pp, n, k, b,
                                 float(vote_radius), _p(out), _p(count), _p(ws), nbytes, _stream()), "ptv3_vote_loss")
    return out, count


def vote_loss_bwd(dloss, votes, coord, target, offset, count, vote_radius):
    """dvotes (N, 3K) fp32 of vote_loss: dloss * mask * clamp((coord + votes) - target, -1, 1) / (3 max(count, 1))."""
    off, n, k, b, tgt, per_point = _vote_args(votes, coord, target, offset)
    _chk(dloss, "dloss", torch.float32)
    _chk(count, "count", torch.int32, 1)
    if dloss.numel() != 1 or count.shape[0] != 1 + k:
        raise RuntimeError("vote_loss_bwd: dloss must hold one value and count 1 + K")
    dvotes = torch.empty_like(votes)
    lib.check(lib.ptv3_vote_loss_bwd(_p(dloss), _p(votes), _p(coord), _p(tgt), per_point, _p(off), _p(count), n, k, b,
                                     float(vote_radius), _p(dvotes), _stream()), "ptv3_vote_loss_bwd")
    return dvotes


# ---------------------------------------------------------------------------------------------
# segmentation losses
# ---------------------------------------------------------------------------------------------
SEG_LOSS_MAX_CLASSES = 1024
NO_IGNORE = -2 ** 63          # ignore_index=None: no label equals it


def seg_loss_capable(n, c):
    """Shapes ptv3_lovasz_* / ptv3_focal_* cover: 2 <= C <= 1024 and N * C < 2^31."""
    return 2 <= c <= SEG_LOSS_MAX_CLASSES and n * c < 2 ** 31


def lovasz_scan_tile():
    return int(lib.ptv3_lovasz_scan_tile())


def _seg_args(who, logits, labels):
    _chk(logits, f"{who}: logits", torch.float32, 2)
    _chk(labels, f"{who}: labels", torch.int64, 1)
    n, c = logits.shape
    if labels.shape[0] != n:
        raise RuntimeError(f"{who}: logits {tuple(logits.shape)} / labels {tuple(labels.shape)}: expected (N, C), (N)")
    return n, c


def lovasz_softmax(logits, labels, ignore_index=None, loss_weight=1.0):
    """Multiclass Lovasz-Softmax of losses/lovasz.py:118-164 + :241-257 without a host read -> (out (1) fp32 = the loss,
    weight (N, C) fp32 in point order, order (C, N) int64 per-class descending order, count (C + 1) int32 = per-class
    foreground counts then the number of present classes)."""
    n, c = _seg_args("lovasz_softmax", logits, labels)
    dev = logits.device
    out = torch.empty(1, dtype=torch.float32, device=dev)
    weight = torch.empty((n, c), dtype=torch.float32, device=dev)
    order = torch.empty((c, n), dtype=torch.int64, device=dev)
    count = torch.empty(c + 1, dtype=torch.int32, device=dev)
    nbytes = lib.ptv3_lovasz_workspace_bytes(n, c)
    ws = _ws(nbytes, dev)
    ign = NO_IGNORE if ignore_index is None else int(ignore_index)
    lib.check(lib.ptv3_lovasz_fwd(_p(logits), _p(labels), n, c, ign, float(loss_weight), _p(out), _p(weight), _p(order),
                                  _p(count), _p(ws), nbytes, _stream()), "ptv3_lovasz_fwd")
    return out, weight, order, count


def lovasz_softmax_bwd(dloss, logits, labels, weight, count, ignore_index=None, loss_weight=1.0):
    """dlogits (N, C) fp32 of lovasz_softmax: the softmax backward with the saved weights."""
    n, c = _seg_args("lovasz_softmax_bwd", logits, labels)
    _chk(dloss, "dloss", torch.float32)
    _chk(weight, "weight", torch.float32, 2)
    _chk(count, "count", torch.int32, 1)
    if dloss.numel() != 1 or tuple(weight.shape) != (n, c) or count.shape[0] != c + 1:
        raise RuntimeError("lovasz_softmax_bwd: dloss must hold one value, weight be (N, C) and count C + 1")
    dlogits = torch.empty_like(logits)
    ign = NO_IGNORE if ignore_index is None else int(ignore_index)
    lib.check(lib.ptv3_lovasz_bwd(_p(dloss), _p(logits), _p(labels), _p(weight), _p(count), n, c, ign,
                                  float(loss_weight), _p(dlogits), _stream()), "ptv3_lovasz_bwd")
    return dlogits


def _focal_alpha(alpha, c):
    _chk(alpha, "alpha", torch.float32, 1)
    if alpha.shape[0] != c:
        raise RuntimeError(f"focal_loss: alpha holds {alpha.shape[0]} values for {c} classes")


def focal_loss(logits, labels, alpha, gamma=2.0, ignore_index=-1, loss_weight=1.0, reduction="mean"):
    """Multi-class sigmoid focal loss of losses/misc.py:123-172 -> (out (1) fp32 = the loss, nvalid (1) int32).
    alpha (C) fp32 on the device."""
    n, c = _seg_args("focal_loss", logits, labels)
    _focal_alpha(alpha, c)
    dev = logits.device
    out = torch.empty(1, dtype=torch.float32, device=dev)
    nvalid = torch.empty(1, dtype=torch.int32, device=dev)
    nbytes = lib.ptv3_focal_workspace_bytes(n, c)
    ws = _ws(nbytes, dev)
    ign = NO_IGNORE if ignore_index is None else int(ignore_index)
    lib.check(lib.ptv3_focal_fwd(_p(logits), _p(labels), _p(alpha), n, c, ign, float(gamma), float(loss_weight),
                                 int(reduction == "mean"), _p(out), _p(nvalid), _p(ws), nbytes, _stream()),
              "ptv3_focal_fwd")
    return out, nvalid


def focal_loss_bwd(dloss, logits, labels, alpha, nvalid, gamma=2.0, ignore_index=-1, loss_weight=1.0, reduction="mean"):
    """dlogits (N, C) fp32 of focal_loss."""
    n, c = _seg_args("focal_loss_bwd", logits, labels)
    _focal_alpha(alpha, c)
    _chk(dloss, "dloss", torch.float32)
    _chk(nvalid, "nvalid", torch.int32, 1)
    if dloss.numel() != 1 or nvalid.numel() != 1:
        raise RuntimeError("focal_loss_bwd: dloss and nvalid must hold one value each")
    dlogits = torch.empty_like(logits)
    ign = NO_IGNORE if ignore_index is None else int(ignore_index)
    lib.check(lib.ptv3_focal_bwd(_p(dloss), _p(logits), _p(labels), _p(alpha), _p(nvalid), n, c, ign, float(gamma),
                                 float(loss_weight), int(reduction == "mean"), _p(dlogits), _stream()), "ptv3_focal_bwd")
    return dlogits


# ---------------------------------------------------------------------------------------------
# context-aware classifier head (csrc/cac.hip)
# ---------------------------------------------------------------------------------------------
def cac_capable(k, c):
    """(K classes, C channels) ptv3_cac_* cover: 2 <= K <= 256, 1 <= C <= 128 and the LDS need within 144 KiB (the six
    shapes of the semseg-cac-v1m1 configs - C 48 / 96, K 20 / 100 / 200 - lie inside)."""
    return bool(lib.ptv3_cac_capable(int(k), int(c)))


def _cac_proto_args(who, x, logits, labels, offset):
    _chk(x, f"{who}: x", torch.float32, 2)
    n, c = x.shape
    if (logits is None) == (labels is None):
        raise RuntimeError(f"{who}: give logits (softmax weights, per scene) or labels (whole batch)")
    if logits is not None:
        _chk(logits, f"{who}: logits", torch.float32, 2)
        if logits.shape[0] != n:
            raise RuntimeError(f"{who}: x {tuple(x.shape)} / logits {tuple(logits.shape)}: expected (N, C), (N, K)")
        off = _scene_offset(offset, "offset")
        return n, c, logits.shape[1], off, off.shape[0]
    _chk(labels, f"{who}: labels", torch.int64, 1)
    if labels.shape[0] != n:
        raise RuntimeError(f"{who}: x {tuple(x.shape)} / labels {tuple(labels.shape)}: expected (N, C), (N)")
    return n, c, None, None, 1


def cac_proto(x, logits=None, labels=None, offset=None, num_classes=None, conf_thresh=0.0):
    """Class prototypes.  logits (N, K) + offset: (proto (B, K, C), den (B, K), None), the confidence-masked softmax
    weighting of post_refine_proto_batch per scene.  labels (N) + num_classes: (proto (K, C), den (K), count (K) int32),
    the label weighting of get_adaptive_perspective over the whole batch."""
    n, c, k, off, b = _cac_proto_args("cac_proto", x, logits, labels, offset)
    k = int(num_classes) if k is None else k
    dev = x.device
    proto = torch.empty((b, k, c), dtype=torch.float32, device=dev)
    den = torch.empty((b, k), dtype=torch.float32, device=dev)
    count = torch.empty(k, dtype=torch.int32, device=dev) if labels is not None else None
    nbytes = lib.ptv3_cac_proto_workspace_bytes(n, k, c, b)
    ws = _ws(nbytes, dev)
    lib.check(lib.ptv3_cac_proto_fwd(_p(x), _p(logits), _p(labels), _p(off), b, n, k, c, float(conf_thresh), _p(proto),
                                     _p(den), _p(count), _p(ws), nbytes, _stream()), "ptv3_cac_proto_fwd")
    if labels is not None:
        return proto[0], den[0], count
    return proto, den, None


def cac_proto_bwd(dproto, den, x_shape, logits=None, labels=None, offset=None, conf_thresh=0.0):
    """dx (N, C) of cac_proto; the weights are recomputed from logits / labels."""
    n, c = x_shape
    _chk(dproto, "dproto", torch.float32)
    _chk(den, "den", torch.float32)
    k = den.shape[-1]
    off, b = None, 1
    if logits is not None:
        _chk(logits, "logits", torch.float32, 2)
        off = _scene_offset(offset, "offset")
        b = off.shape[0]
        if tuple(logits.shape) != (n, k):
            raise RuntimeError("cac_proto_bwd: logits must be (N, K)")
    else:
        _chk(labels, "labels", torch.int64, 1)
        if labels.shape[0] != n:
            raise RuntimeError("cac_proto_bwd: labels must be (N)")
    if dproto.numel() != b * k * c or den.numel() != b * k:
        raise RuntimeError("cac_proto_bwd: dproto must be (B, K, C) and den (B, K)")
    dx = torch.zeros((n, c), dtype=torch.float32, device=dproto.device)
    lib.check(lib.ptv3_cac_proto_bwd(_p(dproto), _p(den), _p(logits), _p(labels), _p(off), b, n, k, c,
                                     float(conf_thresh), _p(dx), _stream()), "ptv3_cac_proto_bwd")
    return dx


def cac_cos_logits(y, q, offset=None, temp=1.0):
    """temp * get_pred(y, q) -> (N, K).  q (B, K, C) with offset: per scene; q (K, C) or (1, K, C): shared."""
    _chk(y, "y", torch.float32, 2)
    _chk(q, "q", torch.float32)
    n, c = y.shape
    shared = q.dim() == 2 or offset is None
    if q.dim() not in (2, 3) or q.shape[-1] != c or (shared and q.dim() == 3 and q.shape[0] != 1):
        raise RuntimeError(f"cac_cos_logits: y {tuple(y.shape)} / q {tuple(q.shape)}: expected (N, C) and (B, K, C) or (K, C)")
    k = q.shape[-2]
    off, b = None, 1
    if not shared:
        off = _scene_offset(offset, "offset")
        b = off.shape[0]
        if q.shape[0] != b:
            raise RuntimeError(f"cac_cos_logits: q holds {q.shape[0]} scenes, offset {b}")
    out = torch.zeros((n, k), dtype=torch.float32, device=y.device) if not shared else \
        torch.empty((n, k), dtype=torch.float32, device=y.device)
    lib.check(lib.ptv3_cac_cos_logits_fwd(_p(y), _p(q), _p(off), b, n, k, c, int(shared), float(temp), _p(out),
                                          _stream()), "ptv3_cac_cos_logits_fwd")
    return out


def cac_distill(pred, soft, labels):
    """get_distill_loss at its defaults -> (out (1) fp32 = the loss, coef (K) fp32, count (K + 1) int32)."""
    n, k = _seg_args("cac_distill", pred, labels)
    _chk(soft, "soft", torch.float32, 2)
    if tuple(soft.shape) != (n, k):
        raise RuntimeError("cac_distill: pred and soft must have one shape")
    dev = pred.device
    out = torch.empty(1, dtype=torch.float32, device=dev)
    coef = torch.empty(k, dtype=torch.float32, device=dev)
    count = torch.empty(k + 1, dtype=torch.int32, device=dev)
    nbytes = lib.ptv3_cac_distill_workspace_bytes(n, k)
    ws = _ws(nbytes, dev)
    lib.check(lib.ptv3_cac_distill_fwd(_p(pred), _p(soft), _p(labels), n, k, _p(out), _p(coef), _p(count), _p(ws),
                                       nbytes, _stream()), "ptv3_cac_distill_fwd")
    return out, coef, count


def cac_distill_bwd(dloss, pred, soft, labels, coef):
    """dpred (N, K) fp32 of cac_distill."""
    n, k = _seg_args("cac_distill_bwd", pred, labels)
    _chk(soft, "soft", torch.float32, 2)
    _chk(dloss, "dloss", torch.float32)
    _chk(coef, "coef", torch.float32, 1)
    if tuple(soft.shape) != (n, k) or dloss.numel() != 1 or coef.shape[0] != k:
        raise RuntimeError("cac_distill_bwd: soft must be (N, K), dloss hold one value and coef K")
    dpred = torch.empty_like(pred)
    lib.check(lib.ptv3_cac_distill_bwd(_p(dloss), _p(pred), _p(soft), _p(labels), _p(coef), n, k, _p(dpred), _stream()),
              "ptv3_cac_distill_bwd")
    return dpred


# ---------------------------------------------------------------------------------------------
# Sonata self-distillation loss (csrc/sonata_loss.hip)
# ---------------------------------------------------------------------------------------------
def sonata_capable(k):
    """K prototypes ptv3_sonata_* cover: 2 <= K <= 4096."""
    return bool(lib.ptv3_sonata_capable(int(k)))


def _sonata_scale(who, value, name):
    value = float(value)
    if not (value > 0.0 and value < float("inf")):
        raise RuntimeError(f"{who}: {name} must be finite and positive, got {value}")
    return value


def _sonata_rows(who, logits, idx, name):
    _chk(logits, f"{who}: {name}", _F, 2)
    _chk(idx, f"{who}: idx_{name}", (torch.int32, torch.int64), 1)
    if logits.shape[0] == 0 and idx.shape[0] > 0:
        raise RuntimeError(f"{who}: {name} has no rows to gather from")
    return int(idx.dtype == torch.int32)


def sonata_sk_pass(x, idx_t, inv_temp, u=None, n_total=None, with_u=True):
    """One Sinkhorn-Knopp sweep over the gathered teacher logits x[idx_t] (never written): (A, u_next), both (K) fp32.
    u None: A[k] = sum_m exp(x[idx_t[m], k] / T).  Otherwise A[k] = sum_m E[m, k] / (n_total d[m]), d = E u.  A is the
    local sum; u_next = 1 / (K A) serves a caller with one rank (None with with_u=False or M = 0).  exp is taken without
    a shift as the reference does: cosine logits and T >= 0.04 keep |x / T| <= 25."""
    who = "sonata_sk_pass"
    i32 = _sonata_rows(who, x, idx_t, "x")
    inv_temp = _sonata_scale(who, inv_temp, "1 / T")
    _chk(u, f"{who}: u", torch.float32, 1)
    nt, k = x.shape
    m = idx_t.shape[0]
    if u is not None and (u.shape[0] != k or n_total is None or n_total < m):
        raise RuntimeError(f"{who}: u must hold K values and n_total count the pairs of all ranks")
    dev = x.device
    if m == 0:
        return torch.zeros(k, dtype=torch.float32, device=dev), None
    a = torch.empty(k, dtype=torch.float32, device=dev)
    u_next = torch.empty(k, dtype=torch.float32, device=dev) if with_u else None
    nbytes = lib.ptv3_sonata_sk_workspace_bytes(m, k)
    ws = _ws(nbytes, dev)
    lib.check(lib.ptv3_sonata_sk_pass(_p(x), _dt(x), _p(idx_t), i32, nt, m, k, inv_temp, _p(u),
                                      float(n_total if u is not None else m), _p(a), _p(u_next), _p(ws), nbytes,
                                      _stream()), "ptv3_sonata_sk_pass")
    return a, u_next


def _sonata_ce_args(who, x, idx_t, u, s, idx_s, offset_s):
    t32 = _sonata_rows(who, x, idx_t, "x")
    s32 = _sonata_rows(who, s, idx_s, "s")
    _chk(u, f"{who}: u", torch.float32, 1)
    off = _scene_offset(offset_s, "offset_s")
    k = x.shape[1]
    if s.shape[1] != k or u.shape[0] != k or idx_s.shape[0] != idx_t.shape[0] or idx_s.shape[0] > s.shape[0]:
        raise RuntimeError(f"{who}: x {tuple(x.shape)} / s {tuple(s.shape)} / u {tuple(u.shape)} / pairs "
                           f"{idx_t.shape[0]}, {idx_s.shape[0]}: expected (Nt, K), (Ns, K), (K) and M <= Ns pairs")
    return t32, s32, off, k


def sonata_ce(x, idx_t, inv_temp, u, s, idx_s, inv_tau, offset_s):
    """The loss of one pairing: (loss (1), d (M), lse (M), gscale (nb)), all fp32.  target[m] = E[m] u / d[m] is formed
    on the fly, log_softmax(s[idx_s[m]] / tau) likewise; pairs are averaged per scene of offset_s (the student's), then
    the scenes up to the last one that has a pair.  idx_s must be strictly increasing.  M = 0: zeros, nothing launched."""
    who = "sonata_ce"
    t32, s32, off, k = _sonata_ce_args(who, x, idx_t, u, s, idx_s, offset_s)
    inv_temp, inv_tau = _sonata_scale(who, inv_temp, "1 / T"), _sonata_scale(who, inv_tau, "1 / tau")
    dev, m, nb = x.device, idx_t.shape[0], off.shape[0]
    if m == 0:
        z = torch.zeros(0, dtype=torch.float32, device=dev)
        return torch.zeros(1, dtype=torch.float32, device=dev), z, z.clone(), torch.zeros(nb, dtype=torch.float32, device=dev)
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    d = torch.empty(m, dtype=torch.float32, device=dev)
    lse = torch.empty(m, dtype=torch.float32, device=dev)
    gscale = torch.empty(nb, dtype=torch.float32, device=dev)
    nbytes = lib.ptv3_sonata_ce_workspace_bytes(m)
    ws = _ws(nbytes, dev)
    lib.check(lib.ptv3_sonata_ce_fwd(_p(x), _dt(x), _p(idx_t), t32, x.shape[0], _p(s), _dt(s), _p(idx_s), s32, s.shape[0],
                                     m, k, inv_temp, inv_tau, _p(u), _p(off), nb, _p(loss), _p(d), _p(lse), _p(gscale),
                                     _p(ws), nbytes, _stream()), "ptv3_sonata_ce_fwd")
    return loss, d, lse, gscale


def sonata_ce_bwd(dloss, x, idx_t, inv_temp, u, s, idx_s, inv_tau, offset_s, d, lse, gscale):
    """ds (Ns, K) in the dtype of s; exact zeros in the rows idx_s leaves out.  The teacher gets no gradient."""
    who = "sonata_ce_bwd"
    t32, s32, off, k = _sonata_ce_args(who, x, idx_t, u, s, idx_s, offset_s)
    inv_temp, inv_tau = _sonata_scale(who, inv_temp, "1 / T"), _sonata_scale(who, inv_tau, "1 / tau")
    m, nb = idx_t.shape[0], off.shape[0]
    for t, name, size in ((dloss, "dloss", 1), (d, "d", m), (lse, "lse", m), (gscale, "gscale", nb)):
        _chk(t, f"{who}: {name}", torch.float32)
        if t.numel() != size:
            raise RuntimeError(f"{who}: {name} must hold {size} values")
    if m == 0:
        return torch.zeros_like(s)
    ds = torch.empty_like(s)
    lib.check(lib.ptv3_sonata_ce_bwd(_p(dloss), _p(x), _dt(x), _p(idx_t), t32, x.shape[0], _p(s), _dt(s), _p(idx_s), s32,
                                     s.shape[0], m, k, inv_temp, inv_tau, _p(u), _p(d), _p(lse), _p(off), nb, _p(gscale),
                                     _p(ds), _stream()), "ptv3_sonata_ce_bwd")
    return ds


# ---------------------------------------------------------------------------------------------
# Concerto image branch (csrc/concerto.hip)
# ---------------------------------------------------------------------------------------------
class ConcertoPlan:
    """Which principal-view rows fall into which image patch (concerto_plan).  u occupied patches; patch_ids (u) int64
    ascending and unique; seg_start (>= u + 1) int32, the pairs of patch j are seg_start[j] .. seg_start[j + 1]; pair_row
    (R * V) int64, the feature row of every pair ordered by (patch, row, view) - entries from seg_start[u] on belong to no
    patch; rows (R) int64 ascending and slot (>= R * V) int64, the patch run of pair (r, v) (>= u: none); n feature rows."""
    __slots__ = ("u", "patch_ids", "seg_start", "pair_row", "rows", "slot", "n", "views")

    def __init__(self, **kw):
        for k, v in kw.items():
            setattr(self, k, v)


def concerto_pool_corr(corr_in, order, seg_start):
    """One pooling level of the pixel correspondences: corr_in (n_in, V, 2) fp32 (an integer tensor is converted once),
    order (n_in) int64 and seg_start (n_out + 1) int32 of the pooling -> (n_out, V, 2) fp32.  Per cluster and view the
    count is over the children with BOTH entries != -1, the sum over ALL children with each -1 entry read as 0, the
    result sum / count or (-1, -1) without a counted child; float64 sums.  V = 0: an empty tensor, nothing launched."""
    who = "concerto_pool_corr"
    if not corr_in.is_floating_point():
        corr_in = corr_in.float()
    _chk(corr_in, f"{who}: corr_in", torch.float32, 3)
    _chk(order, f"{who}: order", torch.int64, 1)
    _chk(seg_start, f"{who}: seg_start", torch.int32, 1)
    n_in, v, two = corr_in.shape
    n_out = seg_start.shape[0] - 1
    if two != 2 or order.shape[0] != n_in or n_out < 0:
        raise RuntimeError(f"{who}: corr_in {tuple(corr_in.shape)} / order {tuple(order.shape)} / seg_start "
                           f"{tuple(seg_start.shape)}: expected (n_in, V, 2), (n_in) and (n_out + 1)")
    out = torch.empty((n_out, v, 2), dtype=torch.float32, device=corr_in.device)
    if v == 0 or n_out == 0 or n_in == 0:
        return out.fill_(-1.0)
    lib.check(lib.ptv3_concerto_pool_corr(_p(corr_in), _p(order), _p(seg_start), n_in, n_out, v, _p(out), _stream()),
              "ptv3_concerto_pool_corr")
    return out


def concerto_plan(corr, rows, scene, img_base, patch_h, patch_w, n_patches, check=False):
    """ConcertoPlan of the final-level correspondences corr (n, V, 2) fp32: rows (R) int64 ascending are the feature rows of
    the principal global views, scene (R) int64 their scenes, img_base (scenes) int64 the first image of each scene.  A
    pair (row, view) is valid when ANY of its two entries is != -1; its patch is (img_base[scene] + view) * patch_h *
    patch_w + trunc(c0) * patch_w + trunc(c1).  ptv3_concerto_pair_keys, the stable ptv3_argsort_i64 and
    ptv3_pool_segments (whose run count is the ONE host read: u), ptv3_concerto_plan_finish.  A patch outside [0, n_patches)
    is a violated precondition; it lands in one bucket with id n_patches, which check=True (one more read) refuses."""
    who = "concerto_plan"
    _chk(corr, f"{who}: corr", torch.float32, 3)
    for t, name in ((rows, "rows"), (scene, "scene"), (img_base, "img_base")):
        _chk(t, f"{who}: {name}", torch.int64, 1)
    n, v, two = corr.shape
    r = rows.shape[0]
    if two != 2 or scene.shape[0] != r or r > n or img_base.shape[0] == 0:
        raise RuntimeError(f"{who}: corr {tuple(corr.shape)} / rows {r} / scene {scene.shape[0]}: expected (n, V, 2) and "
                           "R <= n rows with a scene each")
    dev = corr.device
    if r == 0 or v == 0:
        return ConcertoPlan(u=0, patch_ids=torch.empty(0, dtype=torch.int64, device=dev),
                            seg_start=torch.zeros(1, dtype=torch.int32, device=dev),
                            pair_row=torch.empty(0, dtype=torch.int64, device=dev), rows=rows,
                            slot=torch.empty(0, dtype=torch.int64, device=dev), n=n, views=v)
    key = torch.empty(r * v + 1, dtype=torch.int64, device=dev)
    lib.check(lib.ptv3_concerto_pair_keys(_p(corr), n, _p(rows), _p(scene), r, v, _p(img_base), img_base.shape[0],
                                          int(patch_h), int(patch_w), int(n_patches), _p(key), _stream()),
              "ptv3_concerto_pair_keys")
    order = argsort_codes(key.view(1, -1), 63)[0][0].contiguous()
    slot, seg_start, runs = pool_segments(key, order, 0)
    u = runs - 1                                     # the last run is the one of the pairs without a patch
    patch_ids = torch.empty(u, dtype=torch.int64, device=dev)
    pair_row = torch.empty(r * v, dtype=torch.int64, device=dev)
    lib.check(lib.ptv3_concerto_plan_finish(_p(key), _p(order), _p(seg_start), _p(rows), r, v, u, _p(patch_ids),
                                            _p(pair_row), _stream()), "ptv3_concerto_plan_finish")
    if check and u > 0 and int(patch_ids[-1].item()) >= n_patches:
        raise RuntimeError(f"{who}: a correspondence points outside the {n_patches} patches of the batch's images")
    return ConcertoPlan(u=u, patch_ids=patch_ids, seg_start=seg_start, pair_row=pair_row, rows=rows, slot=slot, n=n,
                        views=v)


def _concerto_plan_rows(who, plan, n):
    if plan.n != n:
        raise RuntimeError(f"{who}: the plan was made for {plan.n} feature rows, got {n}")
    if plan.u == 0:
        raise RuntimeError(f"{who}: no occupied patch (the caller's case, nothing to launch)")


def concerto_patch_mean(feat, plan):
    """mean (u, C) fp32: the mean of feat's rows over the pairs of every occupied patch, added in the plan's order in
    fp32; feat (n, C) fp32 / bf16 is gathered by the kernel, no (pairs, C) copy exists."""
    who = "concerto_patch_mean"
    _chk(feat, f"{who}: feat", _F, 2)
    n, c = feat.shape
    _concerto_plan_rows(who, plan, n)
    mean = torch.empty((plan.u, c), dtype=torch.float32, device=feat.device)
    lib.check(lib.ptv3_concerto_patch_mean_fwd(_p(feat), _dt(feat), n, c, _p(plan.pair_row), _p(plan.seg_start), plan.u,
                                               _p(mean), _stream()), "ptv3_concerto_patch_mean_fwd")
    return mean


def concerto_patch_mean_bwd(dmean, plan, dtype):
    """dfeat (n, C) in `dtype`, every row written: sum over the row's pairs of dmean[slot] / count[slot], zeros for a row
    without a pair."""
    who = "concerto_patch_mean_bwd"
    _chk(dmean, f"{who}: dmean", torch.float32, 2)
    _concerto_plan_rows(who, plan, plan.n)
    if dmean.shape[0] != plan.u or dtype not in _F:
        raise RuntimeError(f"{who}: dmean {tuple(dmean.shape)} for {plan.u} patches, dtype {dtype}")
    c = dmean.shape[1]
    dfeat = torch.empty((plan.n, c), dtype=dtype, device=dmean.device)
    lib.check(lib.ptv3_concerto_patch_mean_bwd(_p(dmean), _p(plan.rows), _p(plan.slot), _p(plan.seg_start), plan.n,
                                               plan.rows.shape[0], plan.views, plan.u, c, _p(dfeat), _dt(dfeat),
                                               _stream()), "ptv3_concerto_patch_mean_bwd")
    return dfeat


def concerto_cos_capable(d):
    """D channels ptv3_concerto_cos_* cover: 1 <= D <= 2048."""
    return bool(lib.ptv3_concerto_cos_capable(int(d)))


def _concerto_cos_args(who, a, b, patch_ids):
    _chk(a, f"{who}: a", _F, 2)
    _chk(b, f"{who}: b", _F, 2)
    _chk(patch_ids, f"{who}: patch_ids", torch.int64, 1)
    if a.shape[1] != b.shape[1] or patch_ids.shape[0] != a.shape[0] or (b.shape[0] == 0 and a.shape[0] > 0):
        raise RuntimeError(f"{who}: a {tuple(a.shape)} / b {tuple(b.shape)} / patch_ids {tuple(patch_ids.shape)}: "
                           "expected (U, D), (patches, D) and (U)")


def concerto_cos(a, b, patch_ids, shift=True):
    """(loss (1), cos (U), stats (U, 4)), all fp32: loss = 10 mean_j (1 - cos(a[j], b[patch_ids[j]])), both rows less
    their mean over D with `shift`, cos as torch.nn.CosineSimilarity(dim=1, eps=1e-6): each norm clamped from below.
    stats = the two means and the two centred norms of every row, float64 sums rounded once."""
    who = "concerto_cos"
    _concerto_cos_args(who, a, b, patch_ids)
    u, d = a.shape
    if u == 0:
        raise RuntimeError(f"{who}: no occupied patch (the caller's case, nothing to launch)")
    dev = a.device
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    cos = torch.empty(u, dtype=torch.float32, device=dev)
    stats = torch.empty((u, 4), dtype=torch.float32, device=dev)
    lib.check(lib.ptv3_concerto_cos_fwd(_p(a), _dt(a), _p(b), _dt(b), _p(patch_ids), u, b.shape[0], d, int(bool(shift)),
                                        _p(cos), _p(stats), _p(loss), _stream()), "ptv3_concerto_cos_fwd")
    return loss, cos, stats


def concerto_cos_bwd(dloss, a, b, patch_ids, shift=True):
    """da (U, D) in a's dtype of dloss * concerto_cos(a, b, patch_ids, shift)[0]; the row statistics are formed again in
    float64 by the kernel; b gets no gradient."""
    who = "concerto_cos_bwd"
    _concerto_cos_args(who, a, b, patch_ids)
    _chk(dloss, f"{who}: dloss", torch.float32)
    u, d = a.shape
    if u == 0 or dloss.numel() != 1:
        raise RuntimeError(f"{who}: dloss must hold one value, for U >= 1 rows")
    da = torch.empty_like(a)
    lib.check(lib.ptv3_concerto_cos_bwd(_p(dloss), _p(a), _dt(a), _p(b), _dt(b), _p(patch_ids), u, b.shape[0], d,
                                        int(bool(shift)), _p(da), _stream()), "ptv3_concerto_cos_bwd")
    return da


# ---------------------------------------------------------------------------------------------
# language-guided head of Point Prompt Training (csrc/ppt_head.hip)
# ---------------------------------------------------------------------------------------------
def ppt_head_capable(c, k):
    """(C channels, K valid classes) ptv3_ppt_head_fwd covers: C a multiple of 16 in [16, 128], 1 <= K <= 256."""
    return bool(lib.ptv3_ppt_head_capable(int(c), int(k)))


def ppt_head_qr(W, b=None):
    """The part of the collapse that depends on proj_head alone, float64 on the host: W (D, C) = Q R (thin) ->
    (R (C, C), q = Q^T b (C), beta = |b - Q q|^2 as a float).  With D < C the factor has D rows only; R and q are
    filled up with zeros to C, which changes no sum of squares."""
    W = W.detach().double().cpu()
    d, c = W.shape
    b = torch.zeros(d, dtype=torch.float64) if b is None else b.detach().double().cpu()
    Q, R = torch.linalg.qr(W, mode="reduced")
    q = Q.t() @ b
    rest = b - Q @ q
    if d < c:
        R = torch.cat([R, torch.zeros(c - d, c, dtype=torch.float64)])
        q = torch.cat([q, torch.zeros(c - d, dtype=torch.float64)])
    return R, q, float(rest @ rest)


def ppt_head_collapse(W, b, E_v, logit_scale, qr=None, dtype=torch.float32):
    """proj_head (W (D, C), b (D) or None), the K valid class embeddings E_v (K, D) and logit_scale -> the operands of
    the collapsed head (include/ptv3_hip.h): (B (C, C + K) = [R^T | M], bias (C + K) = [q | c], beta, s), computed in
    float64 on the host and rounded once to `dtype`, on W's device; beta and s = exp(logit_scale) are floats.
    seg_logits = s * (x B + bias)[:, C:] / sqrt(|(x B + bias)[:, :C]|^2 + beta).  `qr`: a ppt_head_qr(W, b) result
    to reuse (it does not depend on the condition)."""
    R, q, beta = ppt_head_qr(W, b) if qr is None else qr
    W64 = W.detach().double().cpu()
    E64 = E_v.detach().double().cpu()
    b64 = torch.zeros(W64.shape[0], dtype=torch.float64) if b is None else b.detach().double().cpu()
    M = W64.t() @ E64.t()
    c = E64 @ b64
    B = torch.cat([R.t(), M], 1).to(dtype).contiguous().to(W.device)
    bias = torch.cat([q, c]).to(dtype).contiguous().to(W.device)
    s = float(torch.as_tensor(logit_scale).detach().double().exp())
    return B, bias, beta, s


def ppt_head(x, B, bias, beta, s):
    """x (N, C) fp32 and the operands of ppt_head_collapse -> seg_logits (N, K) fp32, one launch."""
    _chk(x, "ppt_head: x", torch.float32, 2)
    _chk(B, "ppt_head: B", torch.float32, 2)
    _chk(bias, "ppt_head: bias", torch.float32, 1)
    n, c = x.shape
    k = B.shape[1] - c
    if B.shape[0] != c or bias.shape[0] != B.shape[1]:
        raise RuntimeError(f"ppt_head: x {tuple(x.shape)} / B {tuple(B.shape)} / bias {tuple(bias.shape)}: expected "
                           "(N, C), (C, C + K), (C + K)")
    out = torch.empty((n, max(k, 0)), dtype=torch.float32, device=x.device)
    lib.check(lib.ptv3_ppt_head_fwd(_p(x), _p(B), _p(bias), float(beta), float(s), n, c, k, _p(out), _stream()),
              "ptv3_ppt_head_fwd")
    return out


# ---------------------------------------------------------------------------------------------
# pointops
# ---------------------------------------------------------------------------------------------
def knn_query(nsample, xyz, offset, new_xyz, new_offset):
    _chk(xyz, "xyz", torch.float32, 2)
    _chk(new_xyz, "new_xyz", torch.float32, 2)
    _chk(offset, "offset", torch.int32, 1)
    _chk(new_offset, "new_offset", torch.int32, 1)
    m = new_xyz.shape[0]
    _check_offsets("knn_query", offset, xyz.shape[0], new_offset, m)
    idx = torch.zeros((m, nsample), dtype=torch.int32, device=xyz.device)
    dist2 = torch.zeros((m, nsample), dtype=torch.float32, device=xyz.device)
    lib.check(lib.ptv3_knn_query(m, int(nsample), _p(xyz), _p(new_xyz), _p(offset), _p(new_offset),
                                 offset.shape[0], _p(idx), _p(dist2), _stream()), "ptv3_knn_query")
    return idx, dist2


# where ptv3_farthest_point_sampling keeps a scene's coordinates and running distances: registers up to FPS_REG_POINTS
# points, LDS for the next FPS_LDS_POINTS, global memory beyond (csrc/fps.hip)
FPS_REG_POINTS = 16384
FPS_LDS_POINTS = 8192


def farthest_point_sampling(xyz, offset, new_offset, ends_host, new_ends_host):
    """idx (m) int32 global rows: farthest point sampling of every scene (ptv3_farthest_point_sampling).  offset /
    new_offset (b) int32 on the device, ends_host / new_ends_host the same numbers as Python lists (the caller has
    them: nothing is read back here); they are checked against the tensors' sizes before any launch."""
    _chk(xyz, "xyz", torch.float32, 2)
    _chk(offset, "offset", torch.int32, 1)
    _chk(new_offset, "new_offset", torch.int32, 1)
    n, b = xyz.shape[0], offset.shape[0]
    if xyz.shape[1] != 3 or new_offset.shape[0] != b or len(ends_host) != b or len(new_ends_host) != b:
        raise ValueError("farthest_point_sampling: xyz must be (n, 3) and the four offset lists of one length")
    sizes = [e - s for s, e in zip([0] + list(ends_host[:-1]), ends_host)]
    counts = [e - s for s, e in zip([0] + list(new_ends_host[:-1]), new_ends_host)]
    if b and (ends_host[-1] != n or min(sizes) < 0 or min(counts) < 0):
        raise ValueError(f"farthest_point_sampling: offsets {list(ends_host)} / {list(new_ends_host)} do not describe "
                         f"{n} points")
    if any(c > 0 and s == 0 for s, c in zip(sizes, counts)):
        raise ValueError("farthest_point_sampling: samples asked of an empty scene")
    if b == 0:    # no scene, nothing to take (the C entry wants at least one)
        if n:
            raise ValueError(f"farthest_point_sampling: {n} points but no scene")
        return torch.zeros(0, dtype=torch.int32, device=xyz.device)
    idx = torch.zeros(new_ends_host[-1], dtype=torch.int32, device=xyz.device)
    tmp = torch.full((n,), 1e10, dtype=torch.float32, device=xyz.device)
    lib.check(lib.ptv3_farthest_point_sampling(b, max(sizes), _p(xyz), _p(offset), _p(new_offset), _p(tmp),
                                               _p(idx), _stream()), "ptv3_farthest_point_sampling")
    return idx


def fold_batchnorm(bn, bias=None):
    """eval BatchNorm1d (or LayerNorm1d) -> per-channel fp32 (scale, shift) from its running statistics; `bias`, the bias
    of the Linear in front of it, is carried into the shift: bn(x + bias) = scale * x + shift."""
    scale = bn.weight.detach().float() * torch.rsqrt(bn.running_var.float() + bn.eps)
    mean = bn.running_mean.float() if bias is None else bn.running_mean.float() - bias.detach().float()
    return scale.contiguous(), (bn.bias.detach().float() - mean * scale).contiguous()


def vector_attention(x_q, x_k, x_v, xyz, idx, w_p1, s_p, t_p, w_p2, b_p2, s_c, t_c, w_w1, s_w, t_w, w_w2, b_w2):
    """out (n, c) fp32: the Point Transformer V1 vector attention over the neighbour rows idx (n, ns) int32 (-1 =
    missing), BatchNorms folded (fold_batchnorm); formulas and weight shapes: ptv3_vector_attn_fwd in
    include/ptv3_hip.h."""
    for t, nm in ((x_q, "x_q"), (x_k, "x_k"), (x_v, "x_v"), (xyz, "xyz")):
        _chk(t, nm, torch.float32, 2)
    _chk(idx, "idx", torch.int32, 2)
    n, c = x_q.shape
    ns, cs = idx.shape[1], c // 8
    if x_k.shape != x_q.shape or x_v.shape != x_q.shape or tuple(xyz.shape) != (n, 3) or idx.shape[0] != n:
        raise RuntimeError("vector_attention: x_q / x_k / x_v (n, c), xyz (n, 3) and idx (n, ns) disagree")
    shapes = ((w_p1, (3, 3)), (s_p, (3,)), (t_p, (3,)), (w_p2, (c, 3)), (b_p2, (c,)), (s_c, (c,)), (t_c, (c,)),
              (w_w1, (cs, c)), (s_w, (cs,)), (t_w, (cs,)), (w_w2, (cs, cs)), (b_w2, (cs,)))
    for k, (t, shape) in enumerate(shapes):
        _chk(t, f"vector_attention weight {k}", torch.float32)
        if c % 8 == 0 and tuple(t.shape) != shape:
            raise RuntimeError(f"vector_attention: weight {k} has shape {tuple(t.shape)}, expected {shape}")
    out = torch.empty_like(x_q)
    lib.check(lib.ptv3_vector_attn_fwd(_p(x_q), _p(x_k), _p(x_v), _p(xyz), _p(idx), n, c, ns,
                                       *[_p(t) for t, _ in shapes], _p(out), _stream()), "ptv3_vector_attn_fwd")
    return out


def _scene_ids(offset, n):
    counts = torch.diff(offset.long(), prepend=offset.new_zeros(1).long())
    return torch.repeat_interleave(torch.arange(offset.shape[0], device=offset.device), counts, output_size=n)


def _check_offsets(what, offset, n, new_offset, m):
    """The kernels trust the scene ends: a wrong last entry walks past the coordinate arrays."""
    ends = torch.stack([offset[-1], new_offset[-1]]).tolist()
    if ends != [n, m] or offset.shape != new_offset.shape:
        raise ValueError(f"{what}: offsets end at {ends} for {n} candidates / {m} queries "
                         f"({offset.shape[0]} / {new_offset.shape[0]} scenes)")


def knn_query_cells(nsample, xyz, offset, new_xyz, new_offset, cell=None):
    """ptv3_knn_query_cells: the neighbours of knn_query by a walk over a uniform grid of edge `cell` (same unit as xyz;
    default: an estimate of the nsample-th neighbour distance from the candidates' bounding box, so that one or two
    shells of cells settle a query).  Rows ascend in (distance, index).  Host syncs: offsets check + grid extent, number
    of occupied cells."""
    _chk(xyz, "xyz", torch.float32, 2)
    _chk(new_xyz, "new_xyz", torch.float32, 2)
    _chk(offset, "offset", torch.int32, 1)
    _chk(new_offset, "new_offset", torch.int32, 1)
    n, m = xyz.shape[0], new_xyz.shape[0]
    dev = xyz.device
    idx = torch.full((m, nsample), -1, dtype=torch.int32, device=dev)
    dist2 = torch.full((m, nsample), 1e10, dtype=torch.float32, device=dev)
    if m == 0 or n == 0:
        return idx, dist2
    _check_offsets("knn_query_cells", offset, n, new_offset, m)
    lo_f = torch.minimum(xyz.amin(0), new_xyz.amin(0))
    hi_f = torch.maximum(xyz.amax(0), new_xyz.amax(0))
    if cell is None:
        # distance to the nsample-th neighbour if the candidates fill their bounding box (r_vol) or lie on a sheet across
        # its largest face (r_surf): a sheet in a thick box makes r_vol too large (cells hold more candidates than
        # needed, still correct), a filled box makes r_surf too small (many shells), hence the clamp
        ext = torch.sort((xyz.amax(0) - xyz.amin(0)).clamp_min(1e-12)).values.tolist()
        r_surf = (nsample * ext[1] * ext[2] / (3.14159 * n)) ** 0.5
        r_vol = (3.0 * nsample * ext[0] * ext[1] * ext[2] / (4 * 3.14159 * n)) ** (1.0 / 3.0)
        cell = max(r_surf, min(r_vol, 4.0 * r_surf), 1e-9)
    cell = float(cell)
    cell_t = torch.full((), cell, dtype=torch.float32, device=dev)
    # cells relative to the bounding box's corner: the quotient stays below the grid extent wherever the scene sits
    # (absolute coordinates far from the origin lose the cell boundary to fp32 rounding: |x / cell| 2^-24 cells)
    csrc = torch.floor((xyz - lo_f) / cell_t).int()
    cq = torch.floor((new_xyz - lo_f) / cell_t).int()
    extent = int(torch.maximum(csrc.amax(), cq.amax()))
    if extent >= 65536:
        raise ValueError(f"knn_query_cells: {extent + 1} cells of edge {cell} along one axis (limit 65536): use a larger cell")
    src_cells = torch.cat([_scene_ids(offset, n).int().unsqueeze(1), csrc], dim=1).contiguous()
    q_cells = torch.cat([_scene_ids(new_offset, m).int().unsqueeze(1), cq], dim=1).contiguous()
    c = src_cells.long()
    key = (((c[:, 0] << 16 | c[:, 1]) << 16 | c[:, 2]) << 16 | c[:, 3]).contiguous()
    order, _, seg_start, ncell = voxel_unique(key)
    uniq = src_cells[order[seg_start[:-1].long()]].contiguous()
    slots = lib.ptv3_subm_table_slots(ncell)
    table = torch.empty(slots * 12, dtype=torch.uint8, device=dev)
    lib.check(lib.ptv3_subm_build_table(_p(uniq), ncell, _p(table), slots, _stream()), "ptv3_subm_build_table")
    lib.check(lib.ptv3_knn_query_cells(m, int(nsample), _p(xyz), _p(new_xyz), _p(q_cells), _p(table), slots, _p(order),
                                       _p(seg_start), _p(offset), cell, _p(idx), _p(dist2), _stream()),
              "ptv3_knn_query_cells")
    return idx, dist2


# ---------------------------------------------------------------------------------------------
# measurement
# ---------------------------------------------------------------------------------------------
FAMILIES = ("linear", "subm_conv", "window_attn", "backward")


_PROFILING = False


def profile_enable(on=True):
    global _PROFILING
    _PROFILING = bool(on)
    lib.check(lib.ptv3_profile_enable(int(on)), "ptv3_profile_enable")


def profile_collect_kernels():
    """{kernel name: dict(ms, flops, bytes, launches)} per KERNEL (one launch per bracket); call before
    profile_collect(), which resets the records."""
    n = int(lib.ptv3_profile_kernel_count())
    ms, fl, by = (ctypes.c_double * n)(), (ctypes.c_double * n)(), (ctypes.c_double * n)()
    la = (ctypes.c_int64 * n)()
    lib.check(lib.ptv3_profile_collect_kernels(ms, fl, by, la), "ptv3_profile_collect_kernels")
    return {lib.ptv3_profile_kernel_name(i).decode(): dict(ms=ms[i], flops=fl[i], bytes=by[i], launches=int(la[i]))
            for i in range(n) if la[i]}


def profile_collect():
    """{family: dict(ms, flops, bytes, launches)} of the device time bracketed by HIP events since enable."""
    n = len(FAMILIES)
    ms, fl, by = (ctypes.c_double * n)(), (ctypes.c_double * n)(), (ctypes.c_double * n)()
    la = (ctypes.c_int64 * n)()
    lib.check(lib.ptv3_profile_collect(ms, fl, by, la), "ptv3_profile_collect")
    return {FAMILIES[i]: dict(ms=ms[i], flops=fl[i], bytes=by[i], launches=int(la[i])) for i in range(n)}


# ---------------------------------------------------------------------------------------------
# OA-CNNs: the kernel-2 / stride-2 sparse conv pair and the adaptive aggregator (fp32)
# ---------------------------------------------------------------------------------------------
def _chk_rows(t, name, cols=None):
    """fp32 (m, C) GPU matrix whose rows may be a column slice of a wider matrix (unit column stride, 16-byte aligned)."""
    if not t.is_cuda or t.dtype != torch.float32 or t.dim() != 2:
        raise TypeError(f"{name}: expected a 2-d float32 GPU tensor")
    if t.stride(1) != 1 or t.stride(0) % 4 or t.storage_offset() % 4 or t.stride(0) < t.shape[1]:
        raise RuntimeError(f"{name}: rows must be contiguous, 16-byte aligned and at a stride that is a multiple of 4")
    if cols is not None and t.shape[1] != cols:
        raise RuntimeError(f"{name}: {t.shape[1]} columns, expected {cols}")


class Down2Plan:
    """Index plan of one SparseConv3d(kernel_size=2, stride=2) and of the SparseInverseConv3d that shares its indice_key:
    parent (n) int32 (-1: the parent lies outside the coarse shape), tap (n) int32, child (m_out, 8) int32, coarse
    (m_out, 4) int32 sites ordered by (b, x, y, z), up_rows (n) int32 = rows sorted by tap, tap_start (10 host ints)."""

    def __init__(self, n, m_out, parent, tap, child, coarse, up_rows, tap_start, out_shape):
        self.n, self.m_out, self.parent, self.tap, self.child, self.coarse = n, m_out, parent, tap, child, coarse
        self.up_rows, self.tap_start, self.out_shape = up_rows, tap_start, out_shape
        self.tap_start_c = (ctypes.c_int32 * 10)(*tap_start)
        self._long = None

    @property
    def dropped(self):
        return self.tap_start[9] - self.tap_start[8]

    def long_indices(self):
        """(child with -1 -> n_in, parent with -1 -> m_out, up_rows, inverse of up_rows) as int64, for torch indexing."""
        if self._long is None:
            child = torch.where(self.child >= 0, self.child, self.n).long()
            parent = torch.where(self.parent >= 0, self.parent, self.m_out).long()
            rows = self.up_rows.long()
            inv = torch.empty_like(rows)
            inv[rows] = torch.arange(self.n, device=rows.device)
            self._long = (child, parent, rows, inv)
        return self._long


def down2_plan(indices, spatial_shape, batch_size):
    """Plan of the strided pair for unique sites `indices` (n, 4) int32 [b, x, y, z]; ONE host read (ten counters)."""
    _chk(indices, "indices", torch.int32, 2)
    n, dev = indices.shape[0], indices.device
    out_shape = [(int(s) - 2) // 2 + 1 for s in spatial_shape]
    if min(out_shape) < 1:
        raise ValueError(f"down2_plan: spatial shape {list(spatial_shape)} is under 2 on some axis")
    none_key = int(batch_size) * out_shape[0] * out_shape[1] * out_shape[2]
    key = torch.empty(n, dtype=torch.int64, device=dev)
    tap = torch.empty(n, dtype=torch.int32, device=dev)
    lib.check(lib.ptv3_down2_keys(_p(indices), n, out_shape[0], out_shape[1], out_shape[2], none_key, _p(key), _p(tap),
                                  _stream()), "ptv3_down2_keys")
    order = argsort_codes(key.view(1, -1), max(1, none_key.bit_length()))[0][0]
    rank = torch.empty(n, dtype=torch.int64, device=dev)
    seg_start = torch.empty(n + 1, dtype=torch.int32, device=dev)
    n_out = torch.empty(1, dtype=torch.int32, device=dev)
    ws_bytes = lib.ptv3_pool_workspace_bytes(n)
    ws = _ws(ws_bytes, dev)
    lib.check(lib.ptv3_pool_segments(_p(key), _p(order), n, 0, None, _p(rank), _p(seg_start), _p(n_out), None, _p(ws),
                                     ws_bytes, _stream()), "ptv3_pool_segments")
    parent = torch.empty(n, dtype=torch.int32, device=dev)
    child = torch.full((n, 8), -1, dtype=torch.int32, device=dev)
    coarse = torch.empty((n, 4), dtype=torch.int32, device=dev)
    up_key = torch.empty(n, dtype=torch.int64, device=dev)
    counts = torch.zeros(10, dtype=torch.int32, device=dev)
    lib.check(lib.ptv3_down2_children(_p(indices), _p(key), _p(tap), _p(rank), _p(order), _p(seg_start), _p(n_out), n,
                                      none_key, _p(parent), _p(child), _p(coarse), _p(up_key), _p(counts), _stream()),
              "ptv3_down2_children")
    up_rows = argsort_codes(up_key.view(1, -1), 4)[0][0].int()
    host = counts.tolist()   # the level's one host read
    tap_start = [0]
    for c in host[1:]:
        tap_start.append(tap_start[-1] + c)
    m_out = host[0]
    return Down2Plan(n, m_out, parent, tap, child[:m_out], coarse[:m_out], up_rows, tap_start, out_shape)


def _epi(bn_scale, bn_shift, cout):
    for t, nm in ((bn_scale, "bn_scale"), (bn_shift, "bn_shift")):
        _chk(t, nm, torch.float32, 1)
        if t is not None and t.numel() != cout:
            raise RuntimeError("epilogue vector length != cout")


def down2_conv(x, w, plan, bn_scale=None, bn_shift=None, act=ACT_NONE):
    """SparseConv3d(kernel_size=2, stride=2): x (n, cin) fp32, w (cout, 2, 2, 2, cin) -> (m_out, cout)."""
    _chk(x, "x", torch.float32, 2)
    _chk(w, "w", torch.float32)
    n, cin = x.shape
    cout = w.shape[0]
    if n != plan.n or w.numel() != cout * 8 * cin:
        raise RuntimeError("down2_conv: shape mismatch")
    _epi(bn_scale, bn_shift, cout)
    out = torch.empty((plan.m_out, cout), dtype=torch.float32, device=x.device)
    lib.check(lib.ptv3_down2_conv(_p(x), _p(w), _p(plan.child), n, plan.m_out, cin, cout, _p(bn_scale), _p(bn_shift),
                                  int(act), _p(out), _stream()), "ptv3_down2_conv")
    return out


def up2_conv(y, w, plan, bn_scale=None, bn_shift=None, act=ACT_NONE):
    """SparseInverseConv3d(kernel_size=2) on the plan of its down conv: y (m_out, cin), w (cout, 2, 2, 2, cin) ->
    (n, cout) on the fine sites in their own order; a site without a parent gets the epilogue of zero."""
    _chk(y, "y", torch.float32, 2)
    _chk(w, "w", torch.float32)
    m, cin = y.shape
    cout = w.shape[0]
    if m != plan.m_out or w.numel() != cout * 8 * cin:
        raise RuntimeError("up2_conv: shape mismatch")
    _epi(bn_scale, bn_shift, cout)
    out = torch.empty((plan.n, cout), dtype=torch.float32, device=y.device)
    lib.check(lib.ptv3_up2_conv(_p(y), _p(w), _p(plan.parent), _p(plan.up_rows), plan.tap_start_c, plan.n, m, cin, cout,
                                _p(bn_scale), _p(bn_shift), int(act), _p(out), _stream()), "ptv3_up2_conv")
    return out


class ClusterPlan:
    """One partition of a level's rows: order (m) int64, seg_start (m + 1) int32, cluster (m) int64 ids, and the cluster
    count on the device (count_dev); count() reads it once, for the taped composition only."""

    def __init__(self, m, order, seg_start, cluster, count_dev):
        self.m, self.order, self.seg_start, self.cluster, self.count_dev = m, order, seg_start, cluster, count_dev
        self._count = None

    def count(self):
        if self._count is None:
            self._count = int(self.count_dev.item())
        return self._count


def cluster_plan(indices, min_xyz, g):
    """voxel_grid(pos, size=g, batch) + torch.unique(return_inverse) of DonwBlock.forward, without a host read."""
    _chk(indices, "indices", torch.int32, 2)
    _chk(min_xyz, "min_xyz", torch.int32, 1)
    m, dev = indices.shape[0], indices.device
    key = torch.empty(m, dtype=torch.int64, device=dev)
    lib.check(lib.ptv3_cluster_keys(_p(indices), m, _p(min_xyz), int(g), _p(key), _stream()), "ptv3_cluster_keys")
    order = argsort_codes(key.view(1, -1), 63)[0][0]
    cluster = torch.empty(m, dtype=torch.int64, device=dev)
    seg_start = torch.empty(m + 1, dtype=torch.int32, device=dev)
    count = torch.empty(1, dtype=torch.int32, device=dev)
    ws_bytes = lib.ptv3_pool_workspace_bytes(m)
    ws = _ws(ws_bytes, dev)
    lib.check(lib.ptv3_pool_segments(_p(key), _p(order), m, 0, None, _p(cluster), _p(seg_start), _p(count), None, _p(ws),
                                     ws_bytes, _stream()), "ptv3_pool_segments")
    return ClusterPlan(m, order, seg_start, cluster, count)


def cluster_center(x, plan):
    """x - clustermean(x)[cluster] (oacnns_v1m1_base.py:92); x may be a column slice."""
    _chk_rows(x, "x")
    m, c = x.shape
    if m != plan.m:
        raise RuntimeError("cluster_center: row count != plan")
    out = torch.empty((m, c), dtype=torch.float32, device=x.device)
    lib.check(lib.ptv3_cluster_center(_p(x), x.stride(0), _p(plan.order), _p(plan.seg_start), _p(plan.count_dev), m, c,
                                      _p(out), _stream()), "ptv3_cluster_center")
    return out


def cluster_softmax_sum(p, v, global_max, plan):
    """agg (m, C), first count rows valid: clustersum(v e) / (clustersum(e) + 1e-6), e = exp(p - global_max) (:94-97)."""
    _chk_rows(p, "p")
    _chk_rows(v, "v", p.shape[1])
    _chk(global_max, "global_max", torch.float32)
    m, c = p.shape
    if m != plan.m or v.shape[0] != m or global_max.numel() != 1:
        raise RuntimeError("cluster_softmax_sum: shape mismatch")
    agg = torch.empty((m, c), dtype=torch.float32, device=p.device)
    lib.check(lib.ptv3_cluster_softmax_sum(_p(p), p.stride(0), _p(v), v.stride(0), _p(global_max), _p(plan.order),
                                           _p(plan.seg_start), _p(plan.count_dev), m, c, _p(agg), _stream()),
              "ptv3_cluster_softmax_sum")
    return agg


def cluster_mix(logits, aggs, plans, head=None):
    """mixed[i] = sum_l softmax(logits[i, :L])[l] * aggs[l][plans[l].cluster[i]] (:99-102).  With `head` (m, C) returns
    cat([head, mixed], 1) in one buffer, the input of `fuse` (:103-104)."""
    if not logits.is_cuda or logits.dtype != torch.float32 or logits.dim() != 2 or logits.stride(1) != 1:
        raise TypeError("logits: expected a 2-d float32 GPU tensor with contiguous rows")   # read value by value
    levels = len(aggs)
    if logits.shape[1] != levels:
        raise RuntimeError("cluster_mix: one logit column per aggregate")
    if len(plans) != levels:
        raise RuntimeError("cluster_mix: one plan per aggregate")
    m = logits.shape[0]
    c = aggs[0].shape[1] if levels else 0
    for a in aggs:
        _chk(a, "agg", torch.float32, 2)
        if a.shape[1] != c or a.shape[0] < m:
            raise RuntimeError("cluster_mix: aggregates must be (m, C)")
    if head is not None:
        _chk_rows(head, "head", c)
    ap = (ctypes.c_void_p * max(levels, 1))(*[a.data_ptr() for a in aggs])
    cp = (ctypes.c_void_p * max(levels, 1))(*[q.cluster.data_ptr() for q in plans])
    ocol = c if head is not None else 0
    out = torch.empty((m, ocol + c), dtype=torch.float32, device=logits.device)
    lib.check(lib.ptv3_cluster_mix(_p(logits), logits.stride(0), ap, cp, levels, _p(head),
                                   head.stride(0) if head is not None else 0, m, c, _p(out), ocol + c, ocol, _stream()),
              "ptv3_cluster_mix")
    return out


def add_act(a, b, act=ACT_NONE):
    """act(a + b) for two fp32 tensors of one shape."""
    _chk(a, "a", torch.float32)
    _chk(b, "b", torch.float32)
    if a.shape != b.shape:
        raise RuntimeError("add_act: shape mismatch")
    out = torch.empty_like(a)
    lib.check(lib.ptv3_add_act(_p(a), _p(b), int(act), _p(out), a.numel(), _stream()), "ptv3_add_act")
    return out


# ---------------------------------------------------------------------------------------------
# SpUNet: the residual-block convolution (fp32)
# ---------------------------------------------------------------------------------------------
def res_conv_capable(m, ca, cb, cout, kvol=27):
    """Whether ptv3_res_conv serves the shape (include/ptv3_hip.h); `ops.res_conv` refuses the others."""
    return bool(lib.ptv3_res_conv_capable(int(m), int(ca), int(cb), int(cout), int(kvol)))


def res_conv_row_tiles(m, cout):
    """16-point row tiles per wave ptv3_res_conv takes at (m, cout): 1 or 2 (which kernel instantiations a shape runs)."""
    return int(lib.ptv3_res_conv_row_tiles(int(m), int(cout)))


def res_conv(xa, w, nbr, xb=None, bn_scale=None, bn_shift=None, res=None, act=ACT_NONE, w_proj=None, proj_scale=None,
             proj_shift=None, row_order=None):
    """out = act(conv3x3x3(cat(xa, xb)) * bn_scale + bn_shift + res), and with w_proj also
    proj = (cat(xa, xb) @ w_proj^T) * proj_scale + proj_shift, in one launch; see ptv3_res_conv in include/ptv3_hip.h.

    Returns out, or (out, proj) when w_proj is given."""
    _chk(xa, "xa", torch.float32, 2)
    _chk(xb, "xb", torch.float32, 2)
    _chk(w, "w", torch.float32)
    _chk(w_proj, "w_proj", torch.float32)
    _chk(nbr, "nbr", torch.int32, 2)
    _chk(row_order, "row_order", torch.int32, 1)
    _chk(res, "res", torch.float32, 2)
    m, ca = xa.shape
    cb = 0 if xb is None else xb.shape[1]
    cout, kvol = w.shape[0], nbr.shape[1]
    if nbr.shape[0] != m or (xb is not None and xb.shape[0] != m):
        raise RuntimeError("res_conv: xa, xb and nbr must have one row per site")
    if w.numel() != cout * kvol * (ca + cb):
        raise RuntimeError(f"res_conv: weight has {w.numel()} elements, expected {cout}x{kvol}x{ca + cb}")
    if w_proj is not None and w_proj.numel() != cout * (ca + cb):
        raise RuntimeError(f"res_conv: w_proj has {w_proj.numel()} elements, expected {cout}x{ca + cb}")
    if w_proj is None and proj_scale is not None:
        raise RuntimeError("res_conv: proj_scale without w_proj")
    _epi(bn_scale, bn_shift, cout)
    _epi(proj_scale, proj_shift, cout)
    if res is not None and tuple(res.shape) != (m, cout):
        raise RuntimeError("res_conv: residual shape mismatch")
    if row_order is not None and row_order.shape[0] != m:
        raise RuntimeError("res_conv: row_order length != m")
    out = torch.empty((m, cout), dtype=torch.float32, device=xa.device)
    proj = torch.empty_like(out) if w_proj is not None else None
    lib.check(lib.ptv3_res_conv(_p(xa), _p(xb), _p(w), _p(nbr), _p(row_order), _p(bn_scale), _p(bn_shift), _p(res),
                                int(act), _p(out), _p(w_proj), _p(proj_scale), _p(proj_shift), _p(proj), m, ca, cb, cout,
                                kvol, _stream()), "ptv3_res_conv")
    return out if proj is None else (out, proj)


# ---------------------------------------------------------------------------------------------
# Point Transformer V2: grouped vector attention, grid pooling
# ---------------------------------------------------------------------------------------------
def grouped_vector_attention(q, k, v, xyz, idx, groups, w_p1, s_p, t_p, w_p2, b_p2, w_w1, s_w, t_w, w_w2, b_w2):
    """out (n, c) fp32: GroupedVectorAttention.forward after the input projections (pe_bias only) over the neighbour rows
    idx (n, ns) int32 (-1 = missing), PointBatchNorms folded (fold_batchnorm); formulas and weight shapes: ptv3_gva_fwd
    in include/ptv3_hip.h."""
    for t, nm in ((q, "q"), (k, "k"), (v, "v"), (xyz, "xyz")):
        _chk(t, nm, torch.float32, 2)
    _chk(idx, "idx", torch.int32, 2)
    n, c = q.shape
    ns, g = idx.shape[1], int(groups)
    if k.shape != q.shape or v.shape != q.shape or tuple(xyz.shape) != (n, 3) or idx.shape[0] != n:
        raise RuntimeError("grouped_vector_attention: q / k / v (n, c), xyz (n, 3) and idx (n, ns) disagree")
    shapes = ((w_p1, (c, 3)), (s_p, (c,)), (t_p, (c,)), (w_p2, (c, c)), (b_p2, (c,)), (w_w1, (g, c)), (s_w, (g,)),
              (t_w, (g,)), (w_w2, (g, g)), (b_w2, (g,)))
    for i, (t, shape) in enumerate(shapes):
        _chk(t, f"grouped_vector_attention weight {i}", torch.float32)
        if g >= 1 and c % g == 0 and tuple(t.shape) != shape:
            raise RuntimeError(f"grouped_vector_attention: weight {i} has shape {tuple(t.shape)}, expected {shape}")
    out = torch.empty_like(q)
    lib.check(lib.ptv3_gva_fwd(_p(q), _p(k), _p(v), _p(xyz), _p(idx), n, c, g, ns, *[_p(t) for t, _ in shapes],
                               _p(out), _stream()), "ptv3_gva_fwd")
    return out


class GridPoolPlan:
    """The partition of one GridPool: cluster (n) int64 = pooled row of every point, order (n) int64 = points sorted by
    cell, seg_start (n_out + 1) int32 = the clusters' runs in `order`, n_out, the pooled cumulative scene ends on the
    device (int64) and on the host, and start (b, 3) = every scene's minimum corner."""

    def __init__(self, cluster, order, seg_start, n_out, offset, offset_host, start):
        self.cluster, self.order, self.seg_start, self.n_out = cluster, order, seg_start, n_out
        self.offset, self.offset_host, self.start = offset, offset_host, start


def grid_pool_plan(coord, offset, size):
    """GridPool.forward's partition (point_transformer_v2m2_base.py:253-275) of coord (n, 3) fp32 with cumulative scene
    ends offset (b) on the device, n >= 1: segment min, voxel_grid, torch.unique(sorted, return_inverse) and torch.sort
    as ptv3_grid_keys + ptv3_argsort_i64 + ptv3_pool_segments.  One host read: the pooled offsets (their last entry is
    the pooled row count) together with the flag of a cell outside the key's 17 bits per axis."""
    _chk(coord, "coord", torch.float32, 2)
    off = _scene_offset(offset, "offset")
    n, b, dev = coord.shape[0], off.shape[0], coord.device
    if coord.shape[1] != 3 or n < 1:
        raise RuntimeError("grid_pool_plan: coord must be (n, 3) with n >= 1")
    start = torch.empty((b, 3), dtype=torch.float32, device=dev)
    key = torch.empty(n, dtype=torch.int64, device=dev)
    batch = torch.empty(n, dtype=torch.int64, device=dev)
    # pooled offsets (b), a scene without points keeps -1; the last slot is the out-of-range flag
    tail = torch.full((b + 1,), -1, dtype=torch.int64, device=dev)
    tail[b] = 0
    lib.check(lib.ptv3_grid_keys(_p(coord), n, _p(off), b, float(size), _p(start), _p(key), _p(batch),
                                 tail.data_ptr() + 8 * b, _stream()), "ptv3_grid_keys")
    order = argsort_codes(key.view(1, -1), 63)[0][0]
    cluster = torch.empty(n, dtype=torch.int64, device=dev)
    seg_start = torch.empty(n + 1, dtype=torch.int32, device=dev)
    n_out = torch.empty(1, dtype=torch.int32, device=dev)
    ws_bytes = lib.ptv3_pool_workspace_bytes(n)
    ws = _ws(ws_bytes, dev)
    lib.check(lib.ptv3_pool_segments(_p(key), _p(order), n, 0, _p(batch), _p(cluster), _p(seg_start), _p(n_out),
                                     _p(tail), _p(ws), ws_bytes, _stream()), "ptv3_pool_segments")
    host = [int(v) for v in tail.tolist()]      # the one read
    if host[b]:
        raise ValueError(f"grid_pool_plan: a scene spans more than {1 << 17} cells of size {size} along an axis")
    host = host[:b]
    if min(host) < 0:
        raise ValueError("grid_pool_plan: a scene without points")
    return GridPoolPlan(cluster, order, seg_start[:host[-1] + 1], host[-1], tail[:b], host, start)


def segment_mean3(coord, order, seg_start, n_out):
    """(n_out, 3) fp32: mean of coord (n, 3) over every run of `order` (segment_csr(coord[order], ptr, "mean"))."""
    _chk(coord, "coord", torch.float32, 2)
    _chk(order, "order", torch.int64, 1)
    _chk(seg_start, "seg_start", torch.int32, 1)
    if coord.shape[1] != 3 or seg_start.shape[0] != n_out + 1:
        raise RuntimeError("segment_mean3: coord (n, 3) and seg_start (n_out + 1) expected")
    out = torch.empty((n_out, 3), dtype=torch.float32, device=coord.device)
    lib.check(lib.ptv3_segment_mean3(_p(coord), _p(order), _p(seg_start), n_out, _p(out), _stream()),
              "ptv3_segment_mean3")
    return out


# ---------------------------------------------------------------------------------------------
# Stratified Transformer (ST-v1m2)
# ---------------------------------------------------------------------------------------------
class StratPlan:
    """The attention plan of one BasicLayer parity: group g has the query rows q_rows[q_ptr[g]:q_ptr[g+1]] (every point
    in exactly one group) and the key rows k_rows[k_ptr[g]:k_ptr[g+1]] (ptv3_strat_cell_keys in include/ptv3_hip.h);
    all four int32 on the device, n_groups and n_keys (= number of (query group, key) slots) on the host."""

    def __init__(self, q_ptr, q_rows, k_ptr, k_rows, n_groups, n_keys, n_windows):
        self.q_ptr, self.q_rows, self.k_ptr, self.k_rows = q_ptr, q_rows, k_ptr, k_rows
        self.n_groups, self.n_keys, self.n_windows = n_groups, n_keys, n_windows

    def edges(self):
        """(index_0, index_1) int64, sorted by query row as BasicLayer.forward leaves them (:441-442): the edge list the
        reference attends over, expanded on the device for the composition and the training path."""
        q_ptr, k_ptr = self.q_ptr.long(), self.k_ptr.long()
        nq, nk = q_ptr[1:] - q_ptr[:-1], k_ptr[1:] - k_ptr[:-1]
        n = self.q_rows.shape[0]
        grp = torch.repeat_interleave(torch.arange(self.n_groups, device=q_ptr.device), nq, output_size=n)
        per_q = nk[grp]                                        # keys of every query, in q_rows order
        m = int(per_q.sum().item())
        qpos = torch.repeat_interleave(torch.arange(n, device=q_ptr.device), per_q, output_size=m)
        first = torch.cumsum(per_q, 0) - per_q
        slot = torch.arange(m, device=q_ptr.device) - first[qpos]
        index_0 = self.q_rows.long()[qpos]
        index_1 = self.k_rows.long()[k_ptr[grp[qpos]] + slot]
        index_0, perm = torch.sort(index_0, stable=True)
        return index_0, index_1[perm]


def stratified_plan(coord, offset, down_idx, window, shifted, coord_min=None):
    """StratPlan of coord (n, 3) fp32 with int32 cumulative scene ends `offset` (b) on the device, for window size
    `window` and the sampled rows down_idx (int32 / int64).  ptv3_strat_cell_keys + ptv3_argsort_i64 + four
    ptv3_pool_segments + ptv3_strat_key_count / _fill; the scans between them are torch.cumsum.  One host read: number of
    groups, of large windows, of key slots, and the flag of a cell outside the key."""
    _chk(coord, "coord", torch.float32, 2)
    _chk(offset, "offset", torch.int32, 1)
    _chk(down_idx, "down_idx", (torch.int32, torch.int64), 1)
    n, b, dev = coord.shape[0], offset.shape[0], coord.device
    if coord.shape[1] != 3 or n < 1:
        raise RuntimeError("stratified_plan: coord must be (n, 3) with n >= 1")
    cmin = (coord.min(0).values if coord_min is None else coord_min).contiguous()
    keys = torch.empty((2, n), dtype=torch.int64, device=dev)     # [key_small, key_large]
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    lib.check(lib.ptv3_strat_cell_keys(_p(coord), n, _p(offset), b, _p(cmin), float(window), int(bool(shifted)),
                                       keys[0].data_ptr(), keys[1].data_ptr(), _p(bad), _stream()),
              "ptv3_strat_cell_keys")
    orders = argsort_codes(keys, 63)[0]
    order_s, order_l = orders[0], orders[1]
    ws_bytes = lib.ptv3_pool_workspace_bytes(n)
    ws = _ws(ws_bytes, dev)

    def segments(which, shift):
        cluster = torch.empty(n, dtype=torch.int64, device=dev)
        seg_start = torch.empty(n + 1, dtype=torch.int32, device=dev)
        n_out = torch.empty(1, dtype=torch.int32, device=dev)
        lib.check(lib.ptv3_pool_segments(keys[which].data_ptr(), orders[which].data_ptr(), n, shift, None, _p(cluster),
                                         _p(seg_start), _p(n_out), None, _p(ws), ws_bytes, _stream()),
                  "ptv3_pool_segments")
        return cluster, seg_start, n_out

    _, q_ptr, n_groups = segments(0, 0)
    cell_of, c_ptr, _ = segments(0, 24)
    lgroup_of, lg_ptr, _ = segments(1, 0)
    window_of, w_ptr, n_windows = segments(1, 27)
    sampled = torch.zeros(n, dtype=torch.uint8, device=dev)
    sampled[down_idx.long()] = 1
    prefix = torch.zeros(n + 1, dtype=torch.int32, device=dev)
    torch.cumsum(sampled[order_l], 0, dtype=torch.int32, out=prefix[1:])
    count = torch.empty(n, dtype=torch.int32, device=dev)
    where = (_p(q_ptr), _p(order_s), _p(cell_of), _p(c_ptr), _p(lgroup_of), _p(lg_ptr), _p(window_of), _p(w_ptr))
    lib.check(lib.ptv3_strat_key_count(*where, _p(prefix), _p(n_groups), n, _p(count), _stream()),
              "ptv3_strat_key_count")
    k_ptr = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    torch.cumsum(count, 0, out=k_ptr[1:])
    g, nw, total, flag = torch.cat([n_groups.long(), n_windows.long(), k_ptr[-1:], bad.long()]).tolist()   # the one read
    if flag:
        raise ValueError(f"stratified_plan: the batch spans more than 512 windows of size {window} along an axis")
    if total >= 1 << 31:
        raise ValueError(f"stratified_plan: {total} key slots do not fit int32")
    k_ptr = k_ptr[:g + 1].int()
    q_ptr = q_ptr[:g + 1]
    s_rows = torch.empty(max(int(down_idx.shape[0]), 1), dtype=torch.int32, device=dev)
    k_rows = torch.empty(total, dtype=torch.int32, device=dev)
    lib.check(lib.ptv3_strat_key_fill(*where, _p(order_l), _p(sampled), _p(prefix), n, g, _p(k_ptr), _p(s_rows),
                                      _p(k_rows), _stream()), "ptv3_strat_key_fill")
    return StratPlan(q_ptr, order_s.int(), k_ptr, k_rows, g, total, nw)


def strat_attn_capable(heads, head_dim, table_rows):
    return bool(lib.ptv3_strat_attn_capable(int(heads), int(head_dim), int(table_rows)))


def strat_pack_tables(table):
    """(2L, heads, head_dim, 3) relative-position table -> (3, 2L, heads, head_dim) fp32 axis-major slabs; once per
    load_state_dict / parameter update (callers cache it on the parameter's version)."""
    return table.detach().float().permute(3, 0, 1, 2).contiguous()


def strat_rel_index(coord, index_0, index_1, window, quant, table_rows):
    """(m, 3) int32: relative_position_index of the pairs (index_0[e], index_1[e]), exactly torch's CPU fp32 values
    (ptv3_strat_rel_index)."""
    _chk(coord, "coord", torch.float32, 2)
    i0, i1 = index_0.int().contiguous(), index_1.int().contiguous()
    _chk(i0, "index_0", torch.int32, 1)
    _chk(i1, "index_1", torch.int32, 1)
    if i0.shape != i1.shape or coord.shape[1] != 3:
        raise RuntimeError("strat_rel_index: index_0 / index_1 (m) and coord (n, 3) expected")
    out = torch.empty((i0.shape[0], 3), dtype=torch.int32, device=coord.device)
    lib.check(lib.ptv3_strat_rel_index(_p(coord), _p(i0), _p(i1), i0.shape[0], float(window), float(quant),
                                       int(table_rows), _p(out), _stream()), "ptv3_strat_rel_index")
    return out


def _check_strat_plan(plan, n):
    """Host check of a plan's ranges (tests and hand-made plans; plans of stratified_plan come from the kernels)."""
    q_ptr, k_ptr = plan.q_ptr.tolist(), plan.k_ptr.tolist()
    g = plan.n_groups
    ok = len(q_ptr) == g + 1 and len(k_ptr) == g + 1 and q_ptr[0] == 0 and k_ptr[0] == 0 and \
        all(a <= b for a, b in zip(q_ptr, q_ptr[1:])) and all(a <= b for a, b in zip(k_ptr, k_ptr[1:])) and \
        q_ptr[-1] <= plan.q_rows.shape[0] and k_ptr[-1] <= plan.k_rows.shape[0]
    for rows in (plan.q_rows, plan.k_rows):
        if rows.numel():
            lo, hi = rows.min().item(), rows.max().item()
            ok = ok and lo >= 0 and hi < n
    if not ok:
        raise ValueError("stratified_attention: the plan's pointers or rows are out of range")


def stratified_attention(qkv, coord, plan, tq, tk, tv, scale, window, quant, out=None, check=False):
    """out (n, heads, head_dim) fp32 = WindowAttention.forward between qkv and proj over the groups of `plan`
    (ptv3_strat_attn_fwd).  qkv (n, 3, heads, head_dim) fp32, the projection's output; tq / tk / tv from
    strat_pack_tables.  Rows that are no query of the plan keep what `out` held (zeros when it is allocated here)."""
    _chk(qkv, "qkv", torch.float32, 4)
    _chk(coord, "coord", torch.float32, 2)
    n, three, heads, hd = qkv.shape
    rows = tq.shape[1]
    for t, nm in ((tq, "tq"), (tk, "tk"), (tv, "tv")):
        _chk(t, nm, torch.float32, 4)
        if tuple(t.shape) != (3, rows, heads, hd):
            raise RuntimeError(f"stratified_attention: {nm} has shape {tuple(t.shape)}, expected {(3, rows, heads, hd)}")
    if three != 3 or tuple(coord.shape) != (n, 3):
        raise RuntimeError("stratified_attention: qkv (n, 3, heads, head_dim) and coord (n, 3) expected")
    if not strat_attn_capable(heads, hd, rows):
        raise NotImplementedError(f"stratified_attention: heads={heads}, head_dim={hd}, table_rows={rows} is not served "
                                  "by ptv3_strat_attn_fwd (head_dim 16, at most 80 table rows)")
    for t, nm in ((plan.q_ptr, "q_ptr"), (plan.q_rows, "q_rows"), (plan.k_ptr, "k_ptr"), (plan.k_rows, "k_rows")):
        _chk(t, nm, torch.int32, 1)
    if plan.q_ptr.shape[0] != plan.n_groups + 1 or plan.k_ptr.shape[0] != plan.n_groups + 1:
        raise RuntimeError("stratified_attention: q_ptr / k_ptr must hold n_groups + 1 entries")
    if check:
        _check_strat_plan(plan, n)
    if out is None:
        out = torch.zeros((n, heads, hd), dtype=torch.float32, device=qkv.device)
    else:
        _chk(out, "out", torch.float32, 3)
        if tuple(out.shape) != (n, heads, hd):
            raise RuntimeError("stratified_attention: out must be (n, heads, head_dim)")
    c = heads * hd
    base = qkv.data_ptr()
    lib.check(lib.ptv3_strat_attn_fwd(base, base + 4 * c, base + 8 * c, 3 * c, _p(coord), _p(tq), _p(tk), _p(tv),
                                      _p(plan.q_ptr), _p(plan.q_rows), _p(plan.k_ptr), _p(plan.k_rows), plan.n_groups,
                                      heads, hd, rows, float(scale), float(window), float(quant), _p(out), _stream()),
              "ptv3_strat_attn_fwd")
    return out


def ball_query(radius, max_neighbor, xyz, offset, ends_host=None):
    """idx (n, max_neighbor) int64: torch_points_kernels.ball_query(..., mode="partial_dense") of a cloud against
    itself (ptv3_ball_query): per row the first max_neighbor rows of its scene within `radius`, in index order, then -1.
    ends_host: the offsets as host integers when the caller has them (otherwise the last one is read back): the kernel
    trusts the scene ends."""
    _chk(xyz, "xyz", torch.float32, 2)
    _chk(offset, "offset", torch.int32, 1)
    n = xyz.shape[0]
    if xyz.shape[1] != 3 or offset.shape[0] < 1:
        raise RuntimeError("ball_query: xyz (n, 3) and at least one scene expected")
    last = int(offset[-1].item()) if ends_host is None else ends_host[-1]
    if last != n or (ends_host is not None and len(ends_host) != offset.shape[0]):
        raise ValueError(f"ball_query: offsets end at {last} for {n} points")
    idx = torch.empty((n, int(max_neighbor)), dtype=torch.int64, device=xyz.device)
    lib.check(lib.ptv3_ball_query(_p(xyz), _p(offset), offset.shape[0], n, float(radius), int(max_neighbor), _p(idx),
                                  _stream()), "ptv3_ball_query")
    return idx


# ---------------------------------------------------------------------------------------------
# OctFormer: the octree of ocnn restated over the library's sort / segment / neighbour kernels, the fused octree
# attention and the block's depthwise conv (parity with ocnn / dwconv unpinned)
# ---------------------------------------------------------------------------------------------
def key_to_xyz(key, depth):
    """(n, 3) int32 cell coordinates and (n) int32 scene ids of octree keys (x in the highest bit of each triple)."""
    xyz = torch.zeros((key.shape[0], 3), dtype=torch.int64, device=key.device)
    for i in range(int(depth)):
        for a in range(3):
            xyz[:, a] |= ((key >> (3 * i + 2 - a)) & 1) << i
    return xyz.int(), (key >> 48).int()


class OctreeLevels:
    """The non-empty nodes of depths min_depth..depth, every tensor in key order: keys[d] (n_d) int64, xyz[d] (n_d, 3)
    int32, batch[d] (n_d) int32, nnum[d] host int, parent[d] (n_d) int64 rows of depth d-1, children[d] (n_d, 8) int32 rows
    of depth d+1 by tap (x&1)*4 + (y&1)*2 + (z&1) (-1: empty), leaf (n points) int64 rows of depth `depth`, features
    (n_depth, C) the leaf means.  Neighbour and deconvolution tables are built on first use."""

    def __init__(self, depth, min_depth, batch_size):
        self.depth, self.min_depth, self.batch_size = depth, min_depth, batch_size
        self.keys, self.xyz, self.batch, self.nnum, self.parent, self.children = {}, {}, {}, {}, {}, {}
        self.leaf = self.features = None
        self._nbr, self._deconv, self._down = {}, {}, {}

    def neighbors(self, d):
        """(n_d, 27) int32, tap (dx+1)*9 + (dy+1)*3 + (dz+1), -1 where the cell is empty."""
        if d not in self._nbr:
            idx = torch.cat([self.batch[d].view(-1, 1), self.xyz[d]], dim=1).contiguous()
            self._nbr[d] = subm_neighbors_blocks(idx, 3)[0]
        return self._nbr[d]

    def deconv_table(self, d):
        """(n_{d+1}, 27) int32 rows of depth d, by the tap of the stride-2 3^3 convolution whose window 2P + {-1, 0, 1}
        holds the fine cell: per axis offset 0 for an even coordinate, +1 for an odd one under its own parent and -1
        for an odd one under the parent's +1 neighbour; -1 elsewhere (at most 8 entries of a row are set)."""
        if d not in self._deconv:
            nbr, par, xyz = self.neighbors(d), self.parent[d + 1], self.xyz[d + 1]
            odd = (xyz & 1).bool()
            tab = torch.full((xyz.shape[0], 27), -1, dtype=torch.int32, device=xyz.device)
            for t in range(27):
                o = (t // 9 - 1, t // 3 % 3 - 1, t % 3 - 1)
                ok = torch.ones(xyz.shape[0], dtype=torch.bool, device=xyz.device)
                src = 0
                for a in range(3):
                    ok &= ~odd[:, a] if o[a] == 0 else odd[:, a]
                    src = src * 3 + (2 if o[a] == -1 else 1)
                tab[:, t] = torch.where(ok, nbr[par, src], tab[:, t])
            self._deconv[d] = tab
        return self._deconv[d]

    def down_plan(self, d):
        """what down2_conv reads of a Down2Plan, for the kernel-2 / stride-2 convolution from depth d to d-1"""
        if d not in self._down:
            self._down[d] = SimpleNamespace(n=self.nnum[d], m_out=self.nnum[d - 1], child=self.children[d - 1])
        return self._down[d]


def octree_build(coord, feat, offset, scale_factor, depth, min_depth):
    """OctreeLevels of ocnn's Octree.build_octree for the points coord (n, 3) fp32 / scale_factor with the features feat
    (n, C) fp32 and the cumulative scene ends offset: ptv3_octree_keys, ONE sort of the leaf keys, one
    ptv3_pool_segments per depth (the parents of sorted keys are runs) and ONE host read (the node counts, the
    out-of-domain flag and the last offset).  A point outside -1 <= p < 1 raises ValueError (the reference would wrap it silently)."""
    _chk(coord, "coord", torch.float32, 2)
    _chk(feat, "feat", torch.float32, 2)
    _chk(offset, "offset", (torch.int32, torch.int64), 1)
    n, dev = coord.shape[0], coord.device
    depth, min_depth = int(depth), int(min_depth)
    if coord.shape[1] != 3 or feat.shape[0] != n or not 1 <= min_depth <= depth <= 16:
        raise RuntimeError("octree_build: coord (n, 3), feat (n, C) and 1 <= min_depth <= depth <= 16 expected")
    num_scenes = offset.shape[0]
    off32 = offset if offset.dtype == torch.int32 else offset.int()
    key = torch.empty(n, dtype=torch.int64, device=dev)
    levels = list(range(depth, min_depth - 1, -1))
    counts = torch.zeros(len(levels) + 1, dtype=torch.int32, device=dev)   # [n_d per level..., flag]
    lib.check(lib.ptv3_octree_keys(_p(coord), _p(off32), num_scenes, n, float(scale_factor), depth, _p(key),
                                   _p(counts) + 4 * len(levels), _stream()), "ptv3_octree_keys")
    order = argsort_codes(key.view(1, -1), 63)[0][0]
    ws_bytes = lib.ptv3_pool_workspace_bytes(n)
    ws = _ws(ws_bytes, dev)
    cluster, seg = {}, {}
    for i, d in enumerate(levels):
        cluster[d] = torch.empty(n, dtype=torch.int64, device=dev)
        seg[d] = torch.empty(n + 1, dtype=torch.int32, device=dev)
        lib.check(lib.ptv3_pool_segments(_p(key), _p(order), n, 3 * (depth - d), None, _p(cluster[d]), _p(seg[d]),
                                         _p(counts) + 4 * i, None, _p(ws), ws_bytes, _stream()), "ptv3_pool_segments")
    host = torch.cat([counts, off32[-1:]]).tolist()   # the forward's one host read
    if host.pop() != n:
        raise ValueError(f"octree_build: the offsets do not end at the {n} points")
    if host[-1]:
        raise ValueError(f"octree_build: a point lies outside -1 <= coord / {scale_factor} < 1 (the octree's domain)")
    oct = OctreeLevels(depth, min_depth, num_scenes)
    for i, d in enumerate(levels):
        n_d = host[i]
        seg[d] = seg[d][:n_d + 1]
        head = order[seg[d][:n_d].long()]
        oct.nnum[d] = n_d
        lead = key[head]
        oct.keys[d] = ((lead >> 48) << 48) | ((lead & ((1 << 48) - 1)) >> (3 * (depth - d)))   # the scene id stays
        oct.xyz[d], oct.batch[d] = key_to_xyz(oct.keys[d], d)
        if d < depth:
            # head of a run of depth d+1 -> its run of depth d
            oct.parent[d + 1] = cluster[d][order[seg[d + 1][:host[i - 1]].long()]]
            child = torch.full((n_d, 8), -1, dtype=torch.int32, device=dev)
            child[oct.parent[d + 1], oct.keys[d + 1] & 7] = torch.arange(host[i - 1], dtype=torch.int32, device=dev)
            oct.children[d] = child
    oct.leaf = cluster[depth]
    cnt = (seg[depth][1:] - seg[depth][:-1]).float().unsqueeze(1)
    oct.features = segment_sum(feat, order, seg[depth], host[0]) / cnt
    return oct


def octree_attention_torch(qkv, xyz, batch, rpe_table, heads, patch, dilation, pos_bnd, scale, pad_row=None):
    """OctreeAttention.forward between qkv and proj (octformer_v1m1_base.py:230-257) as the reference composes it: the
    padded copy (padding rows carry pad_row, the bias of qkv, scene id -1 and coordinates 0), the dilation transpose,
    the gathered RPE, the -1e3 mask and a softmax.  Any device, differentiable: the training and unfused path, and what
    the kernel is tested and measured against."""
    n_t, c3 = qkv.shape
    c, k, d, h = c3 // 3, int(patch), int(dilation), int(heads)
    pad = -n_t % (k * d)
    if pad:
        row = qkv.new_zeros(c3) if pad_row is None else pad_row.to(qkv.dtype)
        qkv = torch.cat([qkv, row.expand(pad, c3)])
        xyz = torch.cat([xyz, xyz.new_zeros((pad, 3))])
        batch = torch.cat([batch, batch.new_full((pad,), -1)])

    data = (qkv.view(-1, k, d, c3).transpose(1, 2) if d > 1 else qkv).reshape(-1, k, c3)
    pos = (xyz.view(-1, k, d, 3).transpose(1, 2) if d > 1 else xyz).reshape(-1, k, 3).long()
    scene = (batch.view(-1, k, d).transpose(1, 2) if d > 1 else batch).reshape(-1, k).long()
    q, key, v = data.reshape(-1, k, 3, h, c // h).permute(2, 0, 3, 1, 4)
    attn = (q * scale) @ key.transpose(-2, -1)
    rel = pos.unsqueeze(2) - pos.unsqueeze(1)
    rpe_num = 2 * pos_bnd + 1
    idx = rel.clamp(-pos_bnd, pos_bnd) + (pos_bnd + torch.arange(3, device=rel.device) * rpe_num)
    bias = rpe_table.index_select(0, idx.reshape(-1)).view(idx.shape + (-1,)).sum(3)
    attn = attn + bias.permute(0, 3, 1, 2)
    mask = scene.unsqueeze(2) - scene.unsqueeze(1)
    attn = attn + mask.masked_fill(mask != 0, -1000).unsqueeze(1)
    out = (torch.softmax(attn, dim=-1) @ v).transpose(1, 2).reshape(-1, c)
    if d > 1:
        out = out.view(-1, d, k, c).transpose(1, 2).reshape(-1, c)
    return out[:n_t]


def octree_attn_capable(c, heads, patch, dilation):
    return bool(lib.ptv3_octree_attn_capable(int(c), int(heads), int(patch), int(dilation)))


def octree_attention(qkv, xyz, batch, rpe_table, heads, patch, dilation, pos_bnd, scale, pad_row=None, fused=True):
    """out (n_t, C) of qkv (n_t, 3C) in node order: ptv3_octree_attn_fwd when it covers the shape and nothing needs a
    gradient (the kernel skips the keys the reference masks with -1e3, so it never reads pad_row), else
    octree_attention_torch."""
    needs_grad = torch.is_grad_enabled() and (qkv.requires_grad or rpe_table.requires_grad)
    if fused and qkv.is_cuda and not needs_grad and qkv.dtype == torch.float32:
        _chk(qkv, "qkv", torch.float32, 2)
        _chk(xyz, "xyz", torch.int32, 2)
        _chk(batch, "batch", torch.int32, 1)
        table = rpe_table.detach()
        _chk(table, "rpe_table", torch.float32, 2)
        n_t, c = qkv.shape[0], qkv.shape[1] // 3
        if qkv.shape[1] != 3 * c or tuple(xyz.shape) != (n_t, 3) or batch.shape[0] != n_t or \
                tuple(table.shape) != (3 * (2 * pos_bnd + 1), heads):
            raise RuntimeError("octree_attention: shape mismatch")
        out = torch.empty((n_t, c), dtype=torch.float32, device=qkv.device)
        rc = lib.ptv3_octree_attn_fwd(_p(qkv), _p(xyz), _p(batch), _p(table), _p(out), n_t, c, int(heads), int(patch),
                                      int(dilation), int(pos_bnd), float(scale), _stream())
        if rc != PTV3_ERR_UNSUPPORTED:   # else: a shape for the composition
            lib.check(rc, "ptv3_octree_attn_fwd")
            return out
    return octree_attention_torch(qkv, xyz, batch, rpe_table, heads, patch, dilation, pos_bnd, scale, pad_row)


def octree_dwconv_torch(x, w, nbr, bn_scale, bn_shift):
    """x + (sum_t w[t] * x[nbr[:, t]]) * bn_scale + bn_shift by one gather per tap (any device, differentiable)."""
    xp = torch.cat([x, x.new_zeros((1, x.shape[1]))])
    idx = torch.where(nbr >= 0, nbr, x.shape[0]).long()
    acc = torch.zeros_like(x)
    for t in range(27):
        acc = acc + xp[idx[:, t]] * w[t]
    return x + (acc * bn_scale + bn_shift)


def octree_dwconv(x, w, nbr, bn_scale, bn_shift):
    """ptv3_octree_dwconv: cpe(data) + data of an OctFormerBlock in eval; w (27, C) or the (27, 1, C) parameter."""
    _chk(x, "x", torch.float32, 2)
    _chk(w, "w", torch.float32)
    _chk(nbr, "nbr", torch.int32, 2)
    _chk(bn_scale, "bn_scale", torch.float32, 1)
    _chk(bn_shift, "bn_shift", torch.float32, 1)
    n, c = x.shape
    if w.numel() != 27 * c or tuple(nbr.shape) != (n, 27) or bn_scale.numel() != c or bn_shift.numel() != c:
        raise RuntimeError("octree_dwconv: shape mismatch")
    out = torch.empty_like(x)
    lib.check(lib.ptv3_octree_dwconv(_p(x), _p(w), _p(nbr), _p(bn_scale), _p(bn_shift), _p(out), n, c, _stream()),
              "ptv3_octree_dwconv")
    return out


# ---------------------------------------------------------------------------------------------
# PointGroup: ball query over a cell grid, on-device clustering, proposals (parity with
# pointgroup_ops unpinned)
# ---------------------------------------------------------------------------------------------
def _pg_args(who, xyz, offsets):
    _chk(xyz, "xyz", torch.float32, 2)
    _chk(offsets, "offsets", torch.int32, 1)
    if xyz.shape[1] != 3 or offsets.shape[0] < 2:
        raise RuntimeError(f"{who}: xyz (n, 3) and offsets (scenes + 1) expected")
    n = xyz.shape[0]
    ws_bytes = lib.ptv3_pg_workspace_bytes(n)
    return n, offsets.shape[0] - 1, torch.empty(ws_bytes, dtype=torch.uint8, device=xyz.device), ws_bytes


def pg_ballquery_batch_p(xyz, batch_idxs, batch_offsets, radius):
    """(idx (nActive) int32, start_len (n, 2) int32) of ptv3_pg_ballquery_batch_p: per point the rows of its scene with
    d2 < radius^2 in ascending index, at most 1000; start = exclusive scan of the counts by point index.  batch_idxs
    may be None.  One synchronisation (the total sizes idx)."""
    n, b, ws, ws_bytes = _pg_args("pg_ballquery_batch_p", xyz, batch_offsets)
    if batch_idxs is not None:
        _chk(batch_idxs, "batch_idxs", torch.int32, 1)
        if batch_idxs.shape[0] != n:
            raise RuntimeError("pg_ballquery_batch_p: batch_idxs must have one entry per point")
    start_len = torch.empty((n, 2), dtype=torch.int32, device=xyz.device)
    total = ctypes.c_int64(0)
    args = (_p(xyz), _p(batch_idxs), _p(batch_offsets), b, n, float(radius), _p(start_len))
    lib.check(lib.ptv3_pg_ballquery_batch_p(*args, None, ctypes.byref(total), _p(ws), ws_bytes, _stream()),
              "ptv3_pg_ballquery_batch_p (count)")
    idx = torch.empty(total.value, dtype=torch.int32, device=xyz.device)
    if total.value:
        lib.check(lib.ptv3_pg_ballquery_batch_p(*args, _p(idx), ctypes.byref(total), _p(ws), ws_bytes, _stream()),
                  "ptv3_pg_ballquery_batch_p (fill)")
    return idx, start_len


def pg_cluster(xyz, label, offsets, radius, min_points, propose_points=0):
    """ptv3_pg_cluster: (cluster_idxs (sum, 2) int32, cluster_offsets (clusters + 1) int32, n_large) on the device, or
    None when a point has more than 1000 neighbours (PTV3_PG_TRUNCATED: the union is not the reference's directed search
    there; take pg_ballquery_batch_p + pg_bfs_cluster_host).  n_large: clusters with more than propose_points members.
    One synchronisation."""
    n, b, ws, ws_bytes = _pg_args("pg_cluster", xyz, offsets)
    _chk(label, "label", torch.int32, 1)
    if label.shape[0] != n:
        raise RuntimeError("pg_cluster: label must have one entry per point")
    cluster_idxs = torch.empty((n, 2), dtype=torch.int32, device=xyz.device)
    cluster_offsets = torch.empty(n + 1, dtype=torch.int32, device=xyz.device)
    record = (ctypes.c_int32 * 4)()
    rc = lib.ptv3_pg_cluster(_p(xyz), _p(label), _p(offsets), b, n, float(radius), int(min_points), int(propose_points),
                             _p(cluster_idxs), _p(cluster_offsets), record, _p(ws), ws_bytes, _stream())
    if rc == PTV3_PG_TRUNCATED:
        return None
    lib.check(rc, "ptv3_pg_cluster")
    return cluster_idxs[:record[1]], cluster_offsets[:record[0] + 1], int(record[3])


def pg_bfs_cluster_host(semantic_label, ball_query_idxs, start_len, threshold):
    """ptv3_pg_bfs_cluster_host on CPU int32 tensors: (cluster_idxs (sum, 2), cluster_offsets (clusters + 1)), members in
    the reference's discovery order.  Touches no GPU."""
    for t, name, dim in ((semantic_label, "semantic_label", 1), (ball_query_idxs, "ball_query_idxs", 1),
                         (start_len, "start_len", 2)):
        if t.is_cuda or t.dtype != torch.int32 or not t.is_contiguous() or t.dim() != dim:
            raise RuntimeError(f"pg_bfs_cluster_host: {name} must be a contiguous {dim}-d CPU int32 tensor")
    n = start_len.shape[0]
    if semantic_label.shape[0] != n or start_len.shape[1] != 2:
        raise RuntimeError("pg_bfs_cluster_host: semantic_label (n) and start_len (n, 2) expected")
    cluster_idxs = torch.empty((n, 2), dtype=torch.int32)
    cluster_offsets = torch.empty(n + 1, dtype=torch.int32)
    counts = (ctypes.c_int32 * 2)()
    rc = lib.ptv3_pg_bfs_cluster_host(_p(semantic_label), _p(ball_query_idxs), ball_query_idxs.shape[0], _p(start_len),
                                      n, int(threshold), _p(cluster_idxs), _p(cluster_offsets), counts)
    if rc != 0:
        raise RuntimeError(f"ptv3_pg_bfs_cluster_host failed (code {rc}): "
                           + ("a list or an entry points outside the arrays" if rc == 2 else "bad argument"))
    return cluster_idxs[:counts[1]].clone(), cluster_offsets[:counts[0] + 1].clone()


def pg_sort_members(cluster_idxs):
    """The lists of pg_bfs_cluster_host with every cluster's members in ascending index (the order pg_cluster writes)."""
    if cluster_idxs.shape[0] == 0:
        return cluster_idxs
    key = cluster_idxs[:, 0].long() * (int(cluster_idxs[:, 1].max()) + 1) + cluster_idxs[:, 1].long()
    return cluster_idxs[torch.argsort(key)].contiguous()


def pg_proposals(cluster_idxs, cluster_offsets, prob, segment_pred, propose_points, num_proposals, row_map=None):
    """ptv3_pg_proposals: (pred_classes (P) int64, pred_scores (P) fp32, pred_masks (P, N) int32) on the device for the
    clusters with more than propose_points members; num_proposals is their number, known to the caller."""
    _chk(cluster_idxs, "cluster_idxs", torch.int32, 2)
    _chk(cluster_offsets, "cluster_offsets", torch.int32, 1)
    _chk(prob, "prob", torch.float32, 2)
    _chk(segment_pred, "segment_pred", torch.int64, 1)
    _chk(row_map, "row_map", torch.int64, 1)
    n, c = prob.shape
    nc = cluster_offsets.shape[0] - 1
    if segment_pred.shape[0] != n or nc < 0 or (cluster_idxs.shape[0] and cluster_idxs.shape[1] != 2):
        raise RuntimeError("pg_proposals: segment_pred (N), cluster_idxs (sum, 2), cluster_offsets (clusters + 1) expected")
    p = int(num_proposals)
    dev = prob.device
    pred_classes = torch.empty(p, dtype=torch.int64, device=dev)
    pred_scores = torch.empty(p, dtype=torch.float32, device=dev)
    pred_masks = torch.empty((p, n), dtype=torch.int32, device=dev)
    slot = torch.empty(max(nc, 1), dtype=torch.int32, device=dev)
    lib.check(lib.ptv3_pg_proposals(_p(cluster_idxs), _p(cluster_offsets), nc, cluster_idxs.shape[0], _p(prob), c,
                                    _p(segment_pred), _p(row_map), 0 if row_map is None else row_map.shape[0], n,
                                    int(propose_points), p, _p(pred_classes), _p(pred_scores), _p(pred_masks), _p(slot),
                                    _stream()), "ptv3_pg_proposals")
    return pred_classes, pred_scores, pred_masks


def pg_head_eval_capable(c, num_classes):
    return bool(lib.ptv3_pg_head_eval_capable(int(c), int(num_classes)))


def pg_head_eval(feat, coord, w1, b1, bn_weight, bn_bias, bn_mean, bn_var, bn_eps, w2, b2, w_seg, b_seg, voxel_size,
                 ignore_index=()):
    """ptv3_pg_head_eval, one launch: (bias_pred (N, 3), logit (N, K), prob (N, K), segment_pred (N) int64, center (N, 3),
    keep (N) bool) from feat (N, C) fp32, C = 64 or 96, K <= 256; weights as torch holds them, BatchNorm by its running
    statistics."""
    _chk(feat, "feat", torch.float32, 2)
    _chk(coord, "coord", torch.float32, 2)
    n, c = feat.shape
    k = w_seg.shape[0]
    if not pg_head_eval_capable(c, k):
        raise RuntimeError(f"pg_head_eval: C = {c} (64 or 96) with {k} classes (1 .. 256) is not built")
    shapes = ((w1, (c, c)), (b1, (c,)), (bn_weight, (c,)), (bn_bias, (c,)), (bn_mean, (c,)), (bn_var, (c,)), (w2, (3, c)),
              (b2, (3,)), (w_seg, (k, c)), (b_seg, (k,)))
    for i, (t, shape) in enumerate(shapes):
        _chk(t, f"pg_head_eval: parameter {i}", torch.float32)
        if tuple(t.shape) != shape:
            raise RuntimeError(f"pg_head_eval: parameter {i} has shape {tuple(t.shape)}, expected {shape}")
    ignore = [int(v) for v in ignore_index]
    if tuple(coord.shape) != (n, 3) or len(ignore) > 8:
        raise RuntimeError("pg_head_eval: coord (N, 3) and at most 8 ignored classes expected")
    dev = feat.device
    bias_pred = torch.empty((n, 3), dtype=torch.float32, device=dev)
    center = torch.empty((n, 3), dtype=torch.float32, device=dev)
    logit = torch.empty((n, k), dtype=torch.float32, device=dev)
    prob = torch.empty((n, k), dtype=torch.float32, device=dev)
    segment_pred = torch.empty(n, dtype=torch.int64, device=dev)
    keep = torch.empty(n, dtype=torch.uint8, device=dev)
    ig = (ctypes.c_int * max(len(ignore), 1))(*ignore)
    lib.check(lib.ptv3_pg_head_eval(_p(feat), _p(coord), n, c, k, _p(w1), _p(b1), _p(bn_weight), _p(bn_bias), _p(bn_mean),
                                    _p(bn_var), float(bn_eps), _p(w2), _p(b2), _p(w_seg), _p(b_seg), float(voxel_size), ig,
                                    len(ignore), _p(bias_pred), _p(logit), _p(prob), _p(segment_pred), _p(center),
                                    _p(keep), _stream()), "ptv3_pg_head_eval")
    return bias_pred, logit, prob, segment_pred, center, keep.bool()


def _pg_loss_args(bias_pred, coord, centroid, instance):
    for t, name in ((bias_pred, "bias_pred"), (coord, "coord"), (centroid, "instance_centroid")):
        _chk(t, name, torch.float32, 2)
        if tuple(t.shape) != (bias_pred.shape[0], 3):
            raise RuntimeError(f"pg_bias_loss: {name} must be (N, 3)")
    _chk(instance, "instance", torch.int64, 1)
    if instance.shape[0] != bias_pred.shape[0]:
        raise RuntimeError("pg_bias_loss: instance must have one entry per point")


def pg_bias_loss(bias_pred, coord, centroid, instance, ignore_index=-1):
    """ptv3_pg_bias_loss_fwd: out (3) fp32 = masked L1 loss, masked negative-cosine loss, their denominator."""
    _pg_loss_args(bias_pred, coord, centroid, instance)
    out = torch.empty(3, dtype=torch.float32, device=bias_pred.device)
    lib.check(lib.ptv3_pg_bias_loss_fwd(_p(bias_pred), _p(coord), _p(centroid), _p(instance), int(ignore_index),
                                        bias_pred.shape[0], _p(out), _stream()), "ptv3_pg_bias_loss_fwd")
    return out


def pg_bias_loss_bwd(dloss, bias_pred, coord, centroid, instance, fwd_out, ignore_index=-1):
    """ptv3_pg_bias_loss_bwd: d bias_pred (N, 3) from dloss (2) = the gradients of the two losses."""
    _pg_loss_args(bias_pred, coord, centroid, instance)
    _chk(dloss, "dloss", torch.float32, 1)
    _chk(fwd_out, "fwd_out", torch.float32, 1)
    if dloss.shape[0] != 2 or fwd_out.shape[0] != 3:
        raise RuntimeError("pg_bias_loss_bwd: dloss (2) and the forward's out (3) expected")
    dbias = torch.empty_like(bias_pred)
    lib.check(lib.ptv3_pg_bias_loss_bwd(_p(dloss), _p(bias_pred), _p(coord), _p(centroid), _p(instance),
                                        int(ignore_index), bias_pred.shape[0], _p(fwd_out), _p(dbias), _stream()),
              "ptv3_pg_bias_loss_bwd")
    return dbias


# ---------------------------------------------------------------------------------------------
# validation hooks (csrc/evaluator.hip)
from .lib import PTV3_F16, PTV3_I32, PTV3_I64, PTV3_U8  # noqa: E402
from .lib import PTV3_SEG_CONFUSION_MAX_K as SEG_CONFUSION_MAX_K, PTV3_INSSEG_MAX_GT as INSSEG_MAX_GT  # noqa: E402

_EV_LOGITS = {torch.float32: PTV3_F32, torch.bfloat16: PTV3_BF16, torch.float16: PTV3_F16}
_EV_INT = {torch.int32: PTV3_I32, torch.int64: PTV3_I64}
_EV_MASK = {torch.int32: PTV3_I32, torch.int64: PTV3_I64, torch.uint8: PTV3_U8, torch.bool: PTV3_U8}
INSSEG_VOID = -2 ** 31        # bit 31 of a code: the point's segment is ignored


def insseg_chunk():
    """Points of one proposal that one workgroup of ptv3_insseg_associate counts."""
    return int(lib.ptv3_insseg_chunk())


def _seg_confusion_args(src, target, k, inverse, counts):
    k = int(k)
    if k < 1:
        raise RuntimeError(f"seg_confusion: {k} classes")
    if src.dim() == 2:
        if src.dtype not in _EV_LOGITS or src.shape[1] != k:
            raise TypeError(f"seg_confusion: logits {tuple(src.shape)} {src.dtype}, expected (N, {k}) fp32 / bf16 / fp16")
    elif src.dim() != 1 or src.dtype not in _EV_INT:
        raise TypeError(f"seg_confusion: src {tuple(src.shape)} {src.dtype}: logits (N, K) or a prediction (N) int32 / "
                        "int64")
    if target.dim() != 1 or target.dtype not in _EV_INT:
        raise TypeError(f"seg_confusion: target {tuple(target.shape)} {target.dtype}, expected (M) int32 / int64")
    if inverse is not None and (inverse.dim() != 1 or inverse.dtype != torch.int64
                                or inverse.shape[0] != target.shape[0]):
        raise TypeError("seg_confusion: inverse must be int64 with one entry per target")
    if inverse is None and target.shape[0] != src.shape[0]:
        raise RuntimeError(f"seg_confusion: {src.shape[0]} rows, {target.shape[0]} targets and no inverse")
    if counts is not None and (counts.dtype != torch.int64 or tuple(counts.shape) != (3, k)
                               or counts.device != src.device):
        raise TypeError(f"seg_confusion: counts must be (3, {k}) int64 on the inputs' device")
    return k


def seg_confusion_torch(src, target, k, ignore_index=-1, inverse=None, counts=None):
    """What seg_confusion counts, composed in torch on the inputs' device (any device): evaluator.py:141-152 with
    misc.py:53-65, the three histograms as bincounts with a spare bin for the values outside [0, K)."""
    k = _seg_confusion_args(src, target, k, inverse, counts)
    if src.dim() == 2:
        cls = torch.arange(k, device=src.device).expand_as(src)
        pred = torch.where(src == src.max(1, keepdim=True)[0], cls, k).min(1)[0]   # lowest index among the maxima
    else:
        pred = src.long()
    if inverse is not None:
        pred = pred[inverse]
    tgt = target.long()
    pred = torch.where(tgt == ignore_index, torch.full_like(pred, int(ignore_index)), pred)

    def hist(x):
        return torch.bincount(torch.where((x >= 0) & (x < k), x, k), minlength=k + 1)[:k]

    out = torch.stack([hist(torch.where(pred == tgt, pred, -1)), hist(pred), hist(tgt)])
    if counts is None:
        return out
    return counts.add_(out)


def seg_confusion(src, target, k, ignore_index=-1, inverse=None, counts=None):
    """ptv3_seg_confusion: counts (3, K) int64 = intersection, predicted area and target area of src - logits (N, K)
    fp32 / bf16 / fp16 or a prediction (N) int32 / int64 - against target (M) int32 / int64, through inverse (M) int64
    when given; added to `counts` when given.  Above SEG_CONFUSION_MAX_K classes the same counts are composed in torch."""
    for t, name in ((src, "src"), (target, "target"), (inverse, "inverse"), (counts, "counts")):
        _chk(t, f"seg_confusion: {name}")
    k = _seg_confusion_args(src, target, k, inverse, counts)
    if k > SEG_CONFUSION_MAX_K:
        return seg_confusion_torch(src, target, k, ignore_index, inverse, counts)
    if counts is None:
        counts = torch.zeros((3, k), dtype=torch.int64, device=src.device)
    n, m = src.shape[0], target.shape[0]
    logits = src.dim() == 2
    pred_ws = torch.empty(n, dtype=torch.int32, device=src.device) if logits and inverse is not None else None
    lib.check(lib.ptv3_seg_confusion(_p(src), (_EV_LOGITS if logits else _EV_INT)[src.dtype], n, _p(inverse), _p(target),
                                     _EV_INT[target.dtype], m, k, int(ignore_index), _p(counts), _p(pred_ws), _stream()),
              "ptv3_seg_confusion")
    return counts


def _insseg_args(masks, code, g, idx):
    g = int(g)
    if masks.dim() != 2 or masks.dtype not in _EV_MASK:
        raise TypeError(f"insseg_associate: masks {tuple(masks.shape)} {masks.dtype}, expected (P, N) int32 / uint8 / "
                        "bool / int64")
    if code.dim() != 1 or code.dtype != torch.int32:
        raise TypeError("insseg_associate: code must be (N) int32")
    if idx is not None and (idx.dim() != 1 or idx.dtype not in _EV_INT or idx.shape[0] != code.shape[0]):
        raise TypeError("insseg_associate: idx must be int32 / int64 with one entry per code")
    if idx is None and masks.shape[1] != code.shape[0]:
        raise RuntimeError(f"insseg_associate: masks of {masks.shape[1]} points, {code.shape[0]} codes and no idx")
    if g < 0:
        raise RuntimeError(f"insseg_associate: {g} ground-truth instances")
    return g


def insseg_associate_torch(masks, code, g, idx=None):
    """What insseg_associate counts, composed in torch on the inputs' device (any device): the set mask, gathered through
    idx, added into the columns of inter by index_add_."""
    g = _insseg_args(masks, code, g, idx)
    on = masks.ne(0)
    if idx is not None:
        on = on[:, idx.long()]
    p = on.shape[0]
    inter = torch.zeros((p, g + 1), dtype=torch.int32, device=masks.device)
    if on.numel():
        inter.index_add_(1, (code & 0x7FFFFFFF).long(), on.to(torch.int32))
    vert = on.sum(1, dtype=torch.int32)
    void = (on & (code < 0)[None]).sum(1, dtype=torch.int32)
    return inter, vert, void


def insseg_associate(masks, code, g, idx=None):
    """ptv3_insseg_associate: (inter (P, G + 1), vert_count (P), void_inter (P)), all int32, of masks (P, Nm) against the
    per-point codes (N) int32 (compact ground-truth index or G, INSSEG_VOID added on a void point).  With idx (N) int32 /
    int64, evaluated point i reads masks[:, idx[i]] (an entry outside [0, Nm) is not set): the map is inverted here, by
    one sort, into the points of every mask column, so that the kernel reads each row once and in order instead of
    gathering from it.  Above INSSEG_MAX_GT instances the same tables are composed in torch."""
    for t, name in ((masks, "masks"), (code, "code"), (idx, "idx")):
        _chk(t, f"insseg_associate: {name}")
    g = _insseg_args(masks, code, g, idx)
    if g > INSSEG_MAX_GT:
        return insseg_associate_torch(masks, code, g, idx)
    p, nm = masks.shape
    n = code.shape[0]
    dev = masks.device
    if p == 0 or n == 0:
        return (torch.zeros((p, g + 1), dtype=torch.int32, device=dev), torch.zeros(p, dtype=torch.int32, device=dev),
                torch.zeros(p, dtype=torch.int32, device=dev))
    col_start = None
    if idx is not None:
        by_column, order = torch.sort(idx)
        code = code[order]
        col_start = torch.searchsorted(by_column, torch.arange(nm + 1, device=dev, dtype=idx.dtype)).int()
    inter = torch.empty((p, g + 1), dtype=torch.int32, device=dev)
    vert = torch.empty(p, dtype=torch.int32, device=dev)
    void = torch.empty(p, dtype=torch.int32, device=dev)
    lib.check(lib.ptv3_insseg_associate(_p(masks), _EV_MASK[masks.dtype], p, nm, _p(col_start), _p(code), n, g, _p(inter),
                                        _p(vert), _p(void), _stream()), "ptv3_insseg_associate")
    return inter, vert, void


# ---------------------------------------------------------------------------------------------
# modulation of every PDBatchNorm of SpUNet-v1m3 in one launch (csrc/pdnorm.hip)
# ---------------------------------------------------------------------------------------------
def pdnorm_capable(c, cc):
    """(layer width C, context width Cc) ptv3_pdnorm_fwd / _bwd cover: 1 <= C <= 4096, 1 <= Cc <= 1024."""
    return bool(lib.ptv3_pdnorm_capable(int(c), int(cc)))


def pdnorm_table(layers):
    """layers: one (W (2C, Cc), b (2C), gamma (C) | None, beta (C) | None, mean (C) | None, var (C) | None) per
    PDBatchNorm, fp32 on one device -> the device table of pointers and channel offsets the kernels walk
    (rows of PTV3_PDNORM_ROW int64), with the host copy of the widths.  The table holds addresses, not values: an in-place update of
    a parameter needs no new table, a parameter replaced by another tensor does (`key` is what to compare)."""
    from .lib import PTV3_PDNORM_ROW
    if len(layers) == 0:
        raise RuntimeError("pdnorm_table: no layers")
    cc = layers[0][0].shape[1]
    rows, widths, offs, off = [], [], [], 0
    for i, (w, b, gamma, beta, mean, var) in enumerate(layers):
        _chk(w, f"pdnorm_table: W[{i}]", torch.float32, 2)
        _chk(b, f"pdnorm_table: b[{i}]", torch.float32, 1)
        c = b.shape[0] // 2
        if w.shape != (2 * c, cc) or b.shape[0] != 2 * c:
            raise RuntimeError(f"pdnorm_table: layer {i}: W {tuple(w.shape)} / b {tuple(b.shape)}, expected (2C, {cc}) / (2C)")
        for t, nm in ((gamma, "gamma"), (beta, "beta"), (mean, "mean"), (var, "var")):
            _chk(t, f"pdnorm_table: {nm}[{i}]", torch.float32, 1)
            if t is not None and t.shape[0] != c:
                raise RuntimeError(f"pdnorm_table: layer {i}: {nm} has {t.shape[0]} entries, expected {c}")
        rows.append([w.data_ptr(), b.data_ptr(), _p(gamma) or 0, _p(beta) or 0, _p(mean) or 0, _p(var) or 0, off, c])
        widths.append(c)
        offs.append(off)
        off += c
    assert len(rows[0]) == PTV3_PDNORM_ROW
    table = torch.tensor(rows, dtype=torch.int64).to(layers[0][0].device)
    return SimpleNamespace(table=table, widths=(ctypes.c_int32 * len(widths))(*widths), width_list=widths, offs=offs,
                           L=len(layers), cc=cc, total=off, key=pdnorm_table_key(layers),
                           has_stats=all(ly[4] is not None and ly[5] is not None for ly in layers),
                           affine=all(ly[2] is not None and ly[3] is not None for ly in layers))


def pdnorm_table_key(layers):
    """the addresses a table of these layers would hold"""
    return tuple(0 if t is None else t.data_ptr() for ly in layers for t in ly)


def pdnorm_fwd(tab, context, fold=False, eps=0.0, save=True):
    """One launch for all layers of `tab`: -> (out0, out1, 1 + scale | None), packed over sum(C) in layer order.
    fold = False: out0 = gamma (1 + scale), out1 = beta (1 + scale) + shift.  fold = True: the same folded with the
    table's running statistics into the (bn_scale, bn_shift) of the conv epilogues."""
    _chk(context, "pdnorm_fwd: context", torch.float32)
    if context.numel() != tab.cc:
        raise RuntimeError(f"pdnorm_fwd: context has {context.numel()} entries, the layers take {tab.cc}")
    dev = context.device
    out0 = torch.empty(tab.total, dtype=torch.float32, device=dev)
    out1 = torch.empty(tab.total, dtype=torch.float32, device=dev)
    one_plus = torch.empty(tab.total, dtype=torch.float32, device=dev) if save else None
    lib.check(lib.ptv3_pdnorm_fwd(_p(tab.table), tab.widths, tab.L, tab.cc, _p(context), int(bool(fold)),
                                  int(tab.has_stats), float(eps), _p(out0), _p(out1), _p(one_plus), _stream()),
              "ptv3_pdnorm_fwd")
    return out0, out1, one_plus


def pdnorm_bwd(tab, context, d_out0, d_out1, one_plus):
    """-> (dW (2 sum C, Cc), db (2 sum C), dgamma (sum C) | None, dbeta (sum C) | None, dcontext (Cc)): layer l's dW / db
    start at row 2 off_l.  Two launches, no atomics."""
    for t, nm in ((context, "context"), (d_out0, "d_out0"), (d_out1, "d_out1"), (one_plus, "one_plus")):
        _chk(t, f"pdnorm_bwd: {nm}", torch.float32)
    if d_out0.numel() != tab.total or d_out1.numel() != tab.total or one_plus.numel() != tab.total:
        raise RuntimeError(f"pdnorm_bwd: the packed gradients must have {tab.total} entries")
    dev = context.device
    dW = torch.empty((2 * tab.total, tab.cc), dtype=torch.float32, device=dev)
    db = torch.empty(2 * tab.total, dtype=torch.float32, device=dev)
    dgamma = torch.empty(tab.total, dtype=torch.float32, device=dev) if tab.affine else None
    dbeta = torch.empty(tab.total, dtype=torch.float32, device=dev) if tab.affine else None
    partial = torch.empty((lib.ptv3_pdnorm_partial_rows(tab.total), tab.cc), dtype=torch.float32, device=dev)
    dctx = torch.empty(tab.cc, dtype=torch.float32, device=dev)
    lib.check(lib.ptv3_pdnorm_bwd(_p(tab.table), tab.widths, tab.L, tab.cc, _p(context), _p(d_out0), _p(d_out1),
                                  _p(one_plus), _p(dW), _p(db), _p(dgamma), _p(dbeta), _p(partial), _p(dctx), _stream()),
              "ptv3_pdnorm_bwd")
    return dW, db, dgamma, dbeta, dctx
