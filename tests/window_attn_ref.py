"""Plain-torch CPU statements of serialized window attention for the kernel tests of csrc/window_attn.hip and
csrc/attn_bwd.hip (no GPU import):

- ramp_qkv: qkv whose log2-domain scores rise along the keys of a window, so that the lazy softmax rescale of the
  resident-window kernel has to run (randn qkv never triggers it);
- attention_f64: the float64 reference (out and log2-domain log-sum-exp), differentiable;
- attention_emulated: the same formula with the roundings window_attn.hip documents for fp32 and bf16, the yardstick
  the tolerances come from;
- rescale_events: a replay of the resident kernel's rescale rule on the reference scores;
- backward_score_sensitivity: how far the rounding of a recomputed score reaches into dq;
- resident_lds_bytes / takes_tiled_kernel / first_tiled_window: the launcher's choice between the resident-window and
  the tiled kernel, restated."""
import math

import numpy as np
import torch

LOG2E = 1.4426950408889634
KEY_TILE = 64          # WA_KT
QUERY_TILE = 16        # rows of one matrix-core tile: the granularity of the rescale decision
RESCALE_THR = 8.0      # WA_RESCALE_THR, log2 units
LDS_LIMIT = 160 * 1024
KINDS = ("randn", "every_tile", "slow", "staircase", "mixed")
_QCHUNK = 1024         # queries evaluated at once (bounds the score matrix of a long window)


def make_plan(sizes, K, seed):
    """A batch of scenes with a seeded random serialization order and the pad plan of patch K.
    Returns dict(n, off, order, inverse, pad, unpad, cu): int64 CPU tensors (cu int32)."""
    from oracle import sfc
    g = torch.Generator().manual_seed(seed)
    off = torch.tensor(sizes).cumsum(0)
    order = torch.cat([torch.randperm(m, generator=g) + (int(off[i]) - m) for i, m in enumerate(sizes)])
    n = int(off[-1])
    inverse = torch.empty_like(order)
    inverse[order] = torch.arange(n)
    pad, unpad, cu = sfc.pad_plan(off.numpy(), K)
    return dict(n=n, off=off, order=order, inverse=inverse, pad=torch.from_numpy(pad), unpad=torch.from_numpy(unpad),
                cu=torch.from_numpy(cu))


def _windows(n_pad, K, cu):
    """{window length: [start, ...]} of the padded slots; uniform windows of K slots when cu is None."""
    if cu is None:
        assert n_pad % K == 0
        return {K: list(range(0, n_pad, K))}
    c = [int(v) for v in cu]
    by_len = {}
    for a, b in zip(c[:-1], c[1:]):
        by_len.setdefault(b - a, []).append(a)
    return by_len


def _slots(n_pad, K, cu):
    """per padded slot: its position inside its window and the window's length"""
    j = torch.empty(n_pad, dtype=torch.int64)
    ln = torch.empty(n_pad, dtype=torch.int64)
    for length, starts in _windows(n_pad, K, cu).items():
        for s in starts:
            j[s:s + length] = torch.arange(length)
            ln[s:s + length] = length
    return j, ln


def ramp_qkv(n, c, heads, order, pad, K, kind, seed, cu=None):
    """qkv (n, 3c) fp32: randn plus, for every head, a shared direction in channel 0: q[:, 0] = 4 * sign(point) and
    k[:, 0] += a(slot).  a is chosen from the point's padded slot j inside its window so that the log2-domain score
    scale * log2(e) * q.k rises by lift(j) units, a step function of the key tile j // 64 (so a partial last key tile
    rises like a full one):
      every_tile  12 units per 64-key tile
      slow        3 units per tile; windows of fewer than 10 key tiles get 27 / (tiles - 1) per tile instead, because
                  two rescales need the score to outgrow the reference by 8 units twice (3 units per tile over the 3
                  later tiles of a 200-key window cannot)
      staircase   flat, +20 from key tile 2 on (tile 1 in windows of at most 3 tiles), +20 more in the last key tile
      mixed       as every_tile, but every third slot has sign -1: its logits fall, its maximum is in tile 0
      randn       nothing added (control)
    A borrowed point sits in two slots; it keeps the amplitude and sign of its own (first) slot."""
    assert kind in KINDS
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(n, 3 * c, generator=g)
    if kind == "randn":
        return qkv
    D = c // heads
    scale = D ** -0.5
    o = order[pad]
    j, ln = _slots(o.shape[0], K, cu)
    tile = j // KEY_TILE
    ntl = (ln + KEY_TILE - 1) // KEY_TILE
    pos = tile.double()
    if kind in ("every_tile", "mixed"):
        lift = 12.0 * pos
    elif kind == "slow":
        rate = torch.maximum(torch.full_like(pos, 3.0), 27.0 / (ntl.clamp(min=2) - 1).double())
        lift = rate * pos
    else:
        first = torch.where(ntl > 3, torch.full_like(ntl, 2), torch.ones_like(ntl))
        lift = 20.0 * (tile >= first).double() + 20.0 * ((tile == ntl - 1) & (ntl > 1)).double()
    sign = torch.ones_like(pos)
    if kind == "mixed":
        sign[j % 3 == 2] = -1.0
    # numpy assigns repeated indices in order (the last one stays): walk the slots backwards so the own slot wins
    amp_pt, sign_pt = np.zeros(n), np.ones(n)
    rev = o.flip(0).numpy()
    amp_pt[rev] = lift.flip(0).numpy()
    sign_pt[rev] = sign.flip(0).numpy()
    unit = 1.0 / (4.0 * scale * LOG2E)   # k[:, 0] amplitude of one log2 unit against q[:, 0] = 4
    for h in range(heads):
        qkv[:, h * D] = torch.from_numpy(4.0 * sign_pt).float()
        qkv[:, c + h * D] += torch.from_numpy(amp_pt * unit).float()
    return qkv


def _round_bf16(t):
    return t.to(torch.bfloat16).to(torch.float32)


def _attend(x, n_pad, heads, K, scale, cu, bias, mode):
    """x (n_pad, 3c) gathered rows -> out (n_pad, c), lse (n_pad, heads) log2 domain.  mode: 'f64', 'f32' or 'bf16'."""
    c = x.shape[1] // 3
    D = c // heads
    dt = torch.float64 if mode == "f64" else torch.float32
    x = x.to(dt)
    if mode == "bf16":
        x = _round_bf16(x)
    out = torch.zeros(n_pad, c, dtype=dt)
    lse = torch.zeros(n_pad, heads, dtype=dt)
    ln2 = math.log(2.0)
    for L, starts in _windows(n_pad, K, cu).items():
        W = len(starts)
        idx = (torch.tensor(starts).unsqueeze(1) + torch.arange(L).unsqueeze(0)).reshape(-1)
        q, k, v = x[idx].reshape(W, L, 3, heads, D).permute(2, 0, 3, 1, 4).unbind(0)      # (W, H, L, D)
        if bias is not None:
            assert cu is None and tuple(bias.shape) == (W, heads, L, L)
        o_parts, l_parts = [], []
        for q0 in range(0, L, _QCHUNK):
            qc = q[:, :, q0:q0 + _QCHUNK]
            b = None if bias is None else bias[:, :, q0:q0 + _QCHUNK].to(dt)
            if mode == "bf16":
                # q' = bf16(q * fp32(scale * log2 e)); scores, maxima and sums fp32; P = bf16(exp2(s - rowmax));
                # the row sum over the rounded P
                qs = _round_bf16(qc * torch.tensor(scale * LOG2E, dtype=torch.float32))
                s = qs @ k.transpose(-2, -1)
                if b is not None:
                    s = s + b * torch.tensor(LOG2E, dtype=torch.float32)
                m = s.max(dim=-1, keepdim=True).values.detach()
                p = _round_bf16(torch.exp2(s - m))
                lsum = p.sum(-1, keepdim=True)
                o_parts.append((p @ v) / lsum)
                l_parts.append((m + torch.log2(lsum)).squeeze(-1))
            else:
                s = (qc * scale) @ k.transpose(-2, -1)
                if b is not None:
                    s = s + b
                l_parts.append(torch.logsumexp(s, dim=-1) / ln2)
                o_parts.append(torch.softmax(s, dim=-1) @ v)
        o_w = torch.cat(o_parts, dim=2)            # (W, H, L, D)
        l_w = torch.cat(l_parts, dim=2)            # (W, H, L)
        out = out.index_copy(0, idx, o_w.transpose(1, 2).reshape(W * L, c))
        lse = lse.index_copy(0, idx, l_w.permute(0, 2, 1).reshape(W * L, heads))
    if mode == "bf16":
        out = _round_bf16(out)
    return out, lse


def attention_f64(qkv, order, inverse, pad, unpad, heads, K, scale, cu=None, bias=None):
    """float64 softmax(scale q k^T [+ bias]) v per window and head, uniform (cu None) or ragged windows.
    Returns out (n, c) and the log2-domain log-sum-exp of every padded slot's row, lse (n_pad, heads).  Differentiable
    in qkv: a borrowed point's gradient is the sum over its two slots."""
    o = order[pad]
    out, lse = _attend(qkv.double()[o], o.shape[0], heads, K, scale, cu, bias, "f64")
    return out[unpad[inverse]], lse


def attention_emulated(qkv, order, inverse, pad, unpad, heads, K, scale, dtype, cu=None, bias=None):
    """attention_f64's formula with the roundings of the kernels: dtype torch.float32 -> everything in torch fp32;
    torch.bfloat16 -> inputs rounded to bf16, q pre-scaled by fp32(scale * log2 e) and rounded to bf16, scores and
    row sums fp32, P = bf16(exp2(s - rowmax)) with the row sum over the rounded P, output rounded to bf16.
    Returns fp32 (out, lse)."""
    o = order[pad]
    mode = "f32" if dtype == torch.float32 else "bf16"
    out, lse = _attend(qkv.float()[o], o.shape[0], heads, K, scale, cu, bias, mode)
    return out[unpad[inverse]], lse


def rescale_events(qkv, order, pad, heads, K, scale, cu=None):
    """Replay of the resident-window kernel's lazy rescale rule on float64 scores.  Per (window, head, 16-query tile):
    after the first key tile has pinned every row's reference to its maximum, a key tile is an event when some row's
    maximum in it exceeds that row's reference by more than RESCALE_THR log2 units; every row of the query tile then
    moves its reference up by max(growth, 0).  Returns (events, later): int64 tensors with one entry per (window,
    head, query tile): the number of events and the number of key tiles after the first."""
    c = qkv.shape[1] // 3
    D = c // heads
    o = order[pad]
    x = qkv.double()[o]
    events, later = [], []
    with torch.no_grad():
        for L, starts in _windows(o.shape[0], K, cu).items():
            W = len(starts)
            ntl = (L + KEY_TILE - 1) // KEY_TILE
            idx = (torch.tensor(starts).unsqueeze(1) + torch.arange(L).unsqueeze(0)).reshape(-1)
            q, k, _ = x[idx].reshape(W, L, 3, heads, D).permute(2, 0, 3, 1, 4).unbind(0)
            step = _QCHUNK                       # a multiple of QUERY_TILE
            for q0 in range(0, L, step):
                s = (q[:, :, q0:q0 + step] * (scale * LOG2E)) @ k.transpose(-2, -1)           # (W, H, R, L)
                R = s.shape[2]
                s = torch.nn.functional.pad(s, (0, ntl * KEY_TILE - L), value=-math.inf)
                tm = s.reshape(W, heads, R, ntl, KEY_TILE).max(-1).values                      # row maxima per key tile
                nqt = (R + QUERY_TILE - 1) // QUERY_TILE
                # rows past the window end hold q = 0: their scores stay at the reference, they never ask for a rescale
                valid = torch.nn.functional.pad(torch.ones(R, dtype=torch.bool), (0, nqt * QUERY_TILE - R))
                tm = torch.nn.functional.pad(tm, (0, 0, 0, nqt * QUERY_TILE - R))
                tm = tm.reshape(W, heads, nqt, QUERY_TILE, ntl)
                valid = valid.reshape(nqt, QUERY_TILE)
                ref = tm[..., 0].clone()
                ev = torch.zeros(W, heads, nqt, dtype=torch.int64)
                for t in range(1, ntl):
                    growth = tm[..., t] - ref
                    hit = ((growth > RESCALE_THR) & valid).any(-1)                             # (W, H, nqt)
                    ev += hit
                    ref = torch.where(hit.unsqueeze(-1), ref + growth.clamp(min=0.0), ref)
                events.append(ev.reshape(-1))
                later.append(torch.full_like(ev, ntl - 1).reshape(-1))
    return torch.cat(events), torch.cat(later)


def backward_score_sensitivity(qkv, dout, order, inverse, pad, unpad, heads, K, scale, cu=None):
    """How far the rounding of a recomputed score reaches into dq, from the float64 reference alone.  A backward that
    recomputes p = exp2(s - lse) from scores carrying independent errors of standard size e (log2 units) has
    dS = p (dP - delta) off by p * ln2 * e * |dP - delta| per pair, and dq[q][c] = scale sum_keys dS k[key][c] by a
    random walk of size scale * ln2 * e * sqrt(sum_keys (p |dP - delta| k[key][c])^2).  (An error of the lse scales a
    whole row of p and leaves sum_keys dS = 0.)  A backward that takes delta = dO . O from the forward's output, as the
    kernels do, does not cancel the common component of k in sum_keys dS = 0, so it really sees that term; autograd
    over one softmax cancels it.
    Returns dict(dq_walk, smax): dq_walk = max over (query, head, channel) of the square root above, smax = max over
    pairs of sum_d |q_d k_d| * scale * log2(e), what a score's partial sums can reach."""
    c = qkv.shape[1] // 3
    D = c // heads
    o = order[pad]
    n_pad = o.shape[0]
    own = unpad[inverse[o]] == torch.arange(n_pad)             # a borrowed duplicate receives no dout
    x = qkv.double()[o]
    do = dout.double()[o] * own.unsqueeze(1)
    res = dict(dq_walk=0.0, smax=0.0)
    with torch.no_grad():
        for L, starts in _windows(n_pad, K, cu).items():
            W = len(starts)
            idx = (torch.tensor(starts).unsqueeze(1) + torch.arange(L).unsqueeze(0)).reshape(-1)
            q, k, v = x[idx].reshape(W, L, 3, heads, D).permute(2, 0, 3, 1, 4).unbind(0)      # (W, H, L, D)
            g = do[idx].reshape(W, L, heads, D).permute(0, 2, 1, 3)
            p = torch.softmax((q * scale) @ k.transpose(-2, -1), dim=-1)
            dp = g @ v.transpose(-2, -1)
            delta = (p * dp).sum(-1, keepdim=True)
            a = p * (dp - delta).abs()
            res["dq_walk"] = max(res["dq_walk"], ((a * a) @ (k * k)).sqrt().max().item())
            res["smax"] = max(res["smax"], ((q.abs() * (scale * LOG2E)) @ k.abs().transpose(-2, -1)).max().item())
    return res


def resident_lds_bytes(esize, head_dim, K):
    """launch_window_attn's lds_full: K rows of head_dim + 4 elements, head_dim V^T rows of Kpad + VPAD elements (VPAD 8
    for 2-byte, 4 for 4-byte elements), Kpad slot indices; Kpad = K rounded up to the key tile."""
    kpad = (K + KEY_TILE - 1) // KEY_TILE * KEY_TILE
    vpad = 8 if esize == 2 else 4
    return (kpad * (head_dim + 4) + head_dim * (kpad + vpad)) * esize + kpad * 4


def takes_tiled_kernel(esize, head_dim, K):
    return resident_lds_bytes(esize, head_dim, K) > LDS_LIMIT


def tiled_lds_bytes(esize, head_dim, K):
    """dynamic LDS of the tiled kernel: one K tile, one V^T tile, K slot indices"""
    return (KEY_TILE * (head_dim + 4) + head_dim * (KEY_TILE + 4)) * esize + K * 4


def first_tiled_window(esize, head_dim):
    """smallest K that is a multiple of the key tile and takes the tiled kernel"""
    K = KEY_TILE
    while not takes_tiled_kernel(esize, head_dim, K):
        K += KEY_TILE
    return K


# ---- the shapes of tests/test_hip_window_attn_paths.py (the CPU tests check the inputs' properties at the same ones)
# resident-window kernel: (C, H, K, scene sizes, ragged plan)
RESIDENT_SHAPES = [
    (32, 2, 1024, [2100], False),           # head_dim 16, 3 windows, the last one borrowing
    (64, 2, 200, [900], False),             # head_dim 32, masked last key tile
    (128, 2, 128, [400], False),            # head_dim 64
    (64, 4, 512, [1500, 70, 700], True),    # ragged; the 70-point scene is one short window
]
# tiled kernel: (element size, C, H, K, scene sizes): K not a multiple of the key tile, 3 windows with a borrowed tail
TILED_SHAPES = [
    (4, 128, 2, 330, [726]),
    (4, 64, 2, 650, [1430]),
    (4, 32, 2, 1160, [2552]),
    (2, 128, 2, 650, [1430]),
    (2, 64, 2, 1230, [2706]),
    (2, 32, 2, 2190, [4500]),
]
RAGGED_EXTRA = 90                           # the short scene appended for the ragged form of a tiled shape
LARGE_SHAPE = (4, 64, 1, 8192, [8193])      # tiled kernel with more than 64 KB of dynamic LDS
