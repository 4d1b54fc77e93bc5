"""CPU statements of LayerNorm (forward, split-K slab input, backward) and of GELU for the kernel tests of csrc/norm.hip,
csrc/backward.hip (layernorm_bwd, act_bwd) and the fused LayerNorms of csrc/block_wide.hip (no GPU import):

- make_inputs / make_bwd_inputs: seeded input families (FAMILIES) for an (m, c) matrix;
- layernorm_f64 / slab_input / layernorm_bwd_f64: float64 references, written out by formula;
- forward_bound / backward_bound: a per-element first-order bound E of what fp32 arithmetic in the kernel's summation
  order may differ from the reference by (derivation below);
- forward_lpr / forward_depth / backward_variant / backward_depth / row_chunks / col_depth: the launchers' choices,
  restated;
- layernorm_emulated / layernorm_bwd_emulated: the kernels' arithmetic in numpy float32, in their summation order, with
  optional seeded defects (FWD_DEFECTS, BWD_DEFECTS): the yardstick that shows E is honest and not slack;
- gelu_f64 / gelu_grad_f64 / gelu_grid: GELU value and derivative in float64 and the grid they are checked on.

The error bound.  u = 2^-24 (half an fp32 ulp, relative).  All inputs are exact fp32 (or bf16) numbers, every operation
below is one rounded fp32 operation, |a (+) b - (a + b)| <= u |a + b|, and terms of order u^2 are dropped except where
stated.  A sum of n numbers whose longest chain of additions is `depth` is off by at most depth * u * sum |terms|.

 1. mean.  s = sum_j x_j by a chain of `depth` additions, mean = s * fl(1 / c): two more roundings (none when c is a
    power of two: 1 / c and the product are exact).
      e_mean = (depth + 2) * u * mean_j |x_j|
 2. centred value d_j = x_j - mean:  |dd_j| <= e_mean + u |d_j|.
 3. variance var = mean_j d_j^2.  The common shift e_mean of all d_j moves sum d_j^2 by 2 e_mean sum d_j + c e_mean^2,
    and sum d_j = 0: only the second-order term e_mean^2 stays (kept: it is what a row of equal values sees).  The
    rounding of d_j (2 u d_j^2), of the square (u d_j^2), of the sum (depth_q, the chain of the squares), of 1 / c and
    the product with it (2 u) and of "+ eps" (u (var + eps)):
      e_var = e_mean^2 + (depth_q + 5) * u * var + u * (var + eps)
 4. rstd = rsqrt(var + eps): relative error  rel_r = e_var / (2 (var + eps)) + RSQRT_U * u, RSQRT_U = 4 for the
    hardware's reciprocal square root (documented to 1 ulp = 2 u; two more for a refinement step's roundings).
 5. xhat_j = d_j * rstd:  e_xhat_j = (e_mean + u |d_j|) * rstd + |xhat_j| * (rel_r + u).
 6. y_j = xhat_j * gamma_j + beta_j + res_j: the product, the two sums:
      E_y = |gamma_j| e_xhat_j + u (|xhat_j gamma_j| + |xhat_j gamma_j + beta_j| + |y_j|)
    The chained second norm reads the stored y (rounded to the output type), so its reference and bound are taken with
    that stored y as the exact input: E_y2 is E_y of a plain LayerNorm.

Backward, g_j = gamma_j dy_j, s1 = mean_j g_j, s2 = mean_j g_j xhat_j, t_j = g_j - s1 - xhat_j s2, dx_j = add_j + rstd t_j:
      e_s1   = (depth + 3) * u * mean_j |g_j|                       (product, chain, 1 / c and its product)
      e_s2   = mean_j |g_j| e_xhat_j + (depth + 4) * u * mean_j |g_j xhat_j|
      e_t_j  = e_s1 + e_xhat_j |s2| + |xhat_j| e_s2 + 3 u (|g_j| + |s1| + |xhat_j s2|)
      E_dx_j = rstd e_t_j + |rstd t_j| (rel_r + u) + u |dx_j|
    column sums over the rows r, col = the chain of one column's sum (col_depth):
      E_dgamma_j = sum_r |dy_rj| e_xhat_rj + (col + 1) * u * sum_r |dy_rj xhat_rj|
      E_dbeta_j  = col * u * sum_r |dy_rj|

The depths restate the launchers: forward, LPR lanes share a row and a lane adds its 4-element chunks one after the
other, (a + b) + (c + d) inside a chunk: depth = 2 + ceil((c / 4) / LPR) + log2(LPR), the squares one by one:
depth_q = 4 ceil((c / 4) / LPR) + log2(LPR).  Packed backward (c / 4 lanes per row, four columns per lane):
2 + log2(c / 4), squares 4 + log2(c / 4).  One-wave backward: NC + 6 for both at most; the additions that have a
nonzero operand are counted (_one_wave_chain), which is what keeps c = 1 and c = 3 testable.
A generic depth = c is 5 to 40 times looser and notices nothing subtle."""
import math

import numpy as np
import torch

U = 2.0 ** -24
RSQRT_U = 4.0
EPS = 1e-5
LN_MAXCH = 8
FAMILIES = ("randn", "offset", "const", "outlier", "tiny", "huge", "small_gamma")
FWD_DEFECTS = ("onepass", "cplus1", "bf16_stats", "no_eps", "gamma_shift", "skip_ragged")
BWD_DEFECTS = ("cplus1", "no_eps", "gamma_shift", "no_s2", "add_twice")

# ---- the shapes of tests/test_hip_norm_paths.py (tests/test_norm_reference_cpu.py checks bound, caps and variant
# coverage at the same ones)
FWD_WIDTHS = (4, 8, 16, 32, 48, 64, 96, 128, 192, 256, 384, 512, 1028, 2048)
FWD_ROWS = (1, 255, 256, 257, 301)
SLAB_WIDTHS = (32, 48, 512)
SLAB_SPLITS = (1, 2, 5)
BWD_WIDTHS = (32, 64, 128, 256, 1, 3, 48, 63, 65, 96, 129, 192, 384, 512, 513, 768, 1024)
BWD_ROWS = (1, 15, 16, 17, 301, 4097)
SWIN_WIDTHS = (48, 96, 192, 384)
FUSED_FAMILIES = ("randn", "offset", "const", "small_gamma")
FUSED_ROWS = (1, 63, 301)


def round_bf16(a):
    """float32 array rounded to the nearest bf16 (ties to even), returned as float32"""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).bfloat16().float().numpy()


def ulp(a, bf16):
    """one unit in the last place of the output type at |a| (elementwise, float64); subnormal spacing below 2^-126"""
    if isinstance(a, torch.Tensor):
        return torch.exp2(torch.floor(torch.log2(a.double().abs().clamp_min(2.0 ** -126))) - (7 if bf16 else 23))
    a = np.abs(np.asarray(a, dtype=np.float64))
    return 2.0 ** (np.floor(np.log2(np.maximum(a, 2.0 ** -126))) - (7 if bf16 else 23))


# ------------------------------------------------------------------------------------------------
# the launchers, restated
# ------------------------------------------------------------------------------------------------
def forward_lpr(c):
    """lanes per row of layernorm_kernel (launch_ln)"""
    nch, lpr = c // 4, 1
    while lpr < 64 and lpr < nch:
        lpr <<= 1
    return lpr


def forward_rounds(c):
    lpr = forward_lpr(c)
    return -(-(c // 4) // lpr)


def forward_depth(c):
    lpr = forward_lpr(c)
    return 2 + forward_rounds(c) + int(math.log2(lpr))


def forward_depth_sq(c):
    return 4 * forward_rounds(c) + int(math.log2(forward_lpr(c)))


def backward_variant(c):
    """'packed' or the NC of layernorm_bwd_kernel (ptv3_layernorm_bwd)"""
    if 32 <= c <= 256 and c & (c - 1) == 0:
        return "packed"
    nc = -(-c // 64)
    for v in (1, 2, 4, 8):
        if nc <= v:
            return v
    return 16


def _one_wave_chain(c):
    """additions with a nonzero operand in the one-wave kernel's row sums: a lane adds its ceil(c / 64) columns one after
    the other, then as many of the 6 butterfly steps as there are lanes with a column (adding an exact 0 does not
    round).  NC + 6 at most; it matters at c = 1 and 3, where every row is (nearly) constant and rstd = eps^-1/2
    multiplies whatever the mean is charged with."""
    return -(-c // 64) - 1 + math.ceil(math.log2(min(c, 64)))


def backward_depth(c):
    v = backward_variant(c)
    return 2 + int(math.log2(c // 4)) if v == "packed" else _one_wave_chain(c)


def backward_depth_sq(c):
    v = backward_variant(c)
    return 4 + int(math.log2(c // 4)) if v == "packed" else _one_wave_chain(c)


def prologue_depth(c):
    """LayerNorm prologue of rows_linear_kernel (csrc/block_wide.hip): a lane adds its c / 4 channels of a row one after
    the other, then the 4 lane groups of the row in 2 butterfly steps; the squares the same way"""
    return c // 4 + 2


def epilogue_depth(cout):
    """LayerNorm epilogue of conv_ln_kernel (csrc/cpe_plus.hip, rows_linear_ln): a lane adds its cout / 16 columns in
    order, then sum16 over the 16 lanes of the row: 4 butterfly steps; the squares the same way"""
    return cout // 16 + 4


def inv_c_roundings(c):
    """roundings of `sum * fl(1 / c)`: none when c is a power of two (1 / c and the product are exact), else two"""
    return 0 if c & (c - 1) == 0 else 2


def row_chunks(m):
    """col_chunks: (rows per chunk, chunks)"""
    r = -(-(-(-m // 256)) // 4) * 4
    r = max(r, 16)
    return r, -(-m // r)


def col_depth(m, c):
    """longest addition chain of one column of dgamma / dbeta: the rows one lane adds inside a chunk, the adds across the
    waves (one-wave kernel: (a + b) + (c + d); packed: its 1024 / c partial rows one after the other), then the slab sum
    (lane z adds chunks z, z + 16, ...; the 16 lane sums are added in order)"""
    rb, ns = row_chunks(m)
    if backward_variant(c) == "packed":
        parts = 1024 // c
        inner = -(-rb // parts) + parts
    else:
        inner = -(-rb // 4) + 2
    return inner + -(-ns // 16) + 16


# ------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------
def make_inputs(family, m, c, seed, bf16=False, offset=100.0):
    """dict(x, res (m, c), gamma, beta, gamma2, beta2 (c)) float32; x and res rounded to bf16 first when bf16.
    offset: the mean of the `offset` family (std 0.5)."""
    assert family in FAMILIES
    g = np.random.default_rng([seed, m, c, FAMILIES.index(family)])
    z = g.standard_normal((m, c))
    if family == "offset":
        x = (offset if c >= 4 else 0.1 * offset) + 0.5 * z       # c < 4: three samples often have a tiny variance
    elif family == "const":
        x = z.copy()
        x[0::2] = 0.4 * (1 + np.arange(x[0::2].shape[0]) % 3)[:, None]      # rows of 0.4, 0.8, 1.2
    elif family == "outlier":
        x = z.copy()
        x[np.arange(m), (7 * np.arange(m)) % c] = 3e4
    elif family == "tiny":
        x = 1e-4 * z
    elif family == "huge":
        x = 3e4 * z + 1e5
    else:
        x = z
    if family == "small_gamma":
        gamma = 10.0 ** g.uniform(-3.0, 3.0, c) * np.where(g.random(c) < 0.5, -1.0, 1.0)
        gamma2 = 10.0 ** g.uniform(-3.0, 3.0, c)
    else:
        gamma = 1.0 + 0.25 * g.standard_normal(c)
        gamma2 = 1.0 + 0.25 * g.standard_normal(c)
    beta = 0.25 * g.standard_normal(c)
    beta2 = 0.25 * g.standard_normal(c)
    res = g.standard_normal((m, c))
    out = dict(x=x, res=res, gamma=gamma, beta=beta, gamma2=gamma2, beta2=beta2)
    out = {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in out.items()}
    if bf16:
        out["x"], out["res"] = round_bf16(out["x"]), round_bf16(out["res"])
    return out


def make_bwd_inputs(family, m, c, seed, bf16=False):
    """make_inputs plus dy and add (m, c)"""
    d = make_inputs(family, m, c, seed, bf16)
    g = np.random.default_rng([seed + 1, m, c])
    d["dy"] = g.standard_normal((m, c)).astype(np.float32)
    d["add"] = g.standard_normal((m, c)).astype(np.float32)
    if bf16:
        d["dy"], d["add"] = round_bf16(d["dy"]), round_bf16(d["add"])
    return d


def slab_input(slabs, bias, bf16):
    """x of layernorm_slabs: the slabs (splits, m, c) added to the bias in slab order in fp32, rounded to the output type"""
    acc = np.broadcast_to(bias.astype(np.float32), slabs.shape[1:]).copy()
    for z in range(slabs.shape[0]):
        acc = acc + slabs[z].astype(np.float32)
    return round_bf16(acc) if bf16 else acc


# ------------------------------------------------------------------------------------------------
# float64 references and bounds
# ------------------------------------------------------------------------------------------------
def _f64(a):
    """float64 of a numpy array or a torch tensor (the references and bounds below use only operators, abs() and
    .mean / .sum, so they run on either; the GPU tests evaluate them in torch float64 on the device)"""
    return a.double() if isinstance(a, torch.Tensor) else np.asarray(a, dtype=np.float64)


def _stats64(x, eps):
    x = _f64(x)
    mean = x.mean(axis=1, keepdims=True)
    d = x - mean
    var = (d * d).mean(axis=1, keepdims=True)
    rstd = (var + eps) ** -0.5
    return x, mean, d, var, rstd


def layernorm_f64(x, gamma, beta, eps=EPS, res=None):
    """y = (x - mean) / sqrt(var + eps) * gamma + beta [+ res], biased variance, float64"""
    x, mean, d, var, rstd = _stats64(x, eps)
    y = d * rstd * _f64(gamma) + _f64(beta)
    if res is not None:
        y = y + _f64(res)
    return y


def _xhat_bound(x, eps, depth, depth_q):
    """steps 1-5: (xhat, rstd, e_xhat, rel_r) in float64"""
    x, mean, d, var, rstd = _stats64(x, eps)
    e_mean = (depth + inv_c_roundings(x.shape[1])) * U * abs(x).mean(axis=1, keepdims=True)
    e_var = e_mean ** 2 + (depth_q + 5) * U * var + U * (var + eps)
    rel_r = e_var / (2.0 * (var + eps)) + RSQRT_U * U
    xhat = d * rstd
    e_xhat = (e_mean + U * abs(d)) * rstd + abs(xhat) * (rel_r + U)
    return xhat, rstd, e_xhat, rel_r


def forward_bound(x, gamma, beta, eps=EPS, res=None, depth=None, depth_q=None):
    """E_y (m, c) float64 of the module docstring; depth / depth_q default to the standalone forward kernel's"""
    c = x.shape[1]
    depth = forward_depth(c) if depth is None else depth
    depth_q = forward_depth_sq(c) if depth_q is None else depth_q
    xhat, rstd, e_xhat, _ = _xhat_bound(x, eps, depth, depth_q)
    gamma = _f64(gamma)
    beta = _f64(beta)
    p = xhat * gamma
    y = p + beta + (0.0 if res is None else _f64(res))
    return abs(gamma) * e_xhat + U * (abs(p) + abs(p + beta) + abs(y))


def layernorm_bwd_f64(x, dy, gamma, eps=EPS, add=None):
    """dx [+ add], dgamma, dbeta in float64:  dx = rstd (g - mean(g) - xhat mean(g xhat)), g = gamma dy"""
    x, mean, d, var, rstd = _stats64(x, eps)
    dy = _f64(dy)
    xhat = d * rstd
    g = dy * _f64(gamma)
    s1 = g.mean(axis=1, keepdims=True)
    s2 = (g * xhat).mean(axis=1, keepdims=True)
    dx = rstd * (g - s1 - xhat * s2)
    if add is not None:
        dx = dx + _f64(add)
    return dx, (dy * xhat).sum(axis=0), dy.sum(axis=0)


def backward_bound(x, dy, gamma, eps=EPS, add=None):
    """(E_dx (m, c), E_dgamma (c), E_dbeta (c)) float64 of the module docstring"""
    m, c = x.shape
    depth, depth_q, col = backward_depth(c), backward_depth_sq(c), col_depth(m, c)
    xhat, rstd, e_xhat, rel_r = _xhat_bound(x, eps, depth, depth_q)
    dy = _f64(dy)
    g = dy * _f64(gamma)
    s1 = g.mean(axis=1, keepdims=True)
    s2 = (g * xhat).mean(axis=1, keepdims=True)
    e_s1 = (depth + 3) * U * abs(g).mean(axis=1, keepdims=True)
    e_s2 = (abs(g) * e_xhat).mean(axis=1, keepdims=True) + (depth + 4) * U * abs(g * xhat).mean(axis=1, keepdims=True)
    t = g - s1 - xhat * s2
    e_t = e_s1 + e_xhat * abs(s2) + abs(xhat) * e_s2 + 3 * U * (abs(g) + abs(s1) + abs(xhat * s2))
    dx = rstd * t + (0.0 if add is None else _f64(add))
    e_dx = rstd * e_t + abs(rstd * t) * (rel_r + U) + U * abs(dx)
    e_dg = (abs(dy) * e_xhat).sum(axis=0) + (col + 1) * U * abs(dy * xhat).sum(axis=0)
    e_db = col * U * abs(dy).sum(axis=0)
    return e_dx, e_dg, e_db


# ------------------------------------------------------------------------------------------------
# fp32 emulation in the kernels' summation order
# ------------------------------------------------------------------------------------------------
F = np.float32


def _butterfly(v):
    """__shfl_xor reduction over the last axis (a power of two): every lane ends with the same sum"""
    n, d = v.shape[-1], 1
    idx = np.arange(n)
    while d < n:
        v = v + v[..., idx ^ d]
        d <<= 1
    return v[..., :1]


def _rsqrt(a):
    with np.errstate(divide="ignore", invalid="ignore"):
        return (F(1.0) / np.sqrt(a.astype(F))).astype(F)


def _fwd_stats(v, valid, c, eps, defect, src=None):
    """v (m, K, LPR, 4) float32 in the kernel's chunk layout (chunk = sub + k * LPR), valid (K, LPR)
    -> mean, rstd (m, 1, 1, 1)"""
    K = v.shape[1]
    s_src = v if src is None else src
    use = valid.copy()
    if defect == "skip_ragged":
        use &= valid.all(axis=1, keepdims=True)         # a round in which not every lane has a chunk is left out
    inv_c = F(1.0) / F(c + 1 if defect == "cplus1" else c)
    s = np.zeros(v.shape[:1] + v.shape[2:3], dtype=F)
    for k in range(K):
        t = (s_src[:, k, :, 0] + s_src[:, k, :, 1]) + (s_src[:, k, :, 2] + s_src[:, k, :, 3])
        s = np.where(use[k], s + t, s)
    mean = (_butterfly(s) * inv_c)[:, None, :, None]    # (m, 1, 1, 1)
    q = np.zeros_like(s)
    for k in range(K):
        for e in range(4):
            if defect == "onepass":
                t = s_src[:, k, :, e] * s_src[:, k, :, e]
            else:
                dd = s_src[:, k, :, e] - mean[:, 0, :, 0]
                t = dd * dd
            q = np.where(use[k], q + t, q)
    var = (_butterfly(q) * inv_c)[:, None, :, None]
    if defect == "onepass":
        var = var - mean * mean
    rstd = _rsqrt(var if defect == "no_eps" else var + F(eps))
    return mean, rstd


def _fwd_layout(a, c):
    """(m, c) -> (m, K, LPR, 4) zero padded, and the (K, LPR) mask of real chunks"""
    lpr, K = forward_lpr(c), forward_rounds(c)
    m, nch = a.shape[0], c // 4
    pad = np.zeros((m, K * lpr * 4), dtype=F)
    pad[:, :c] = a
    valid = (np.arange(K * lpr) < nch).reshape(K, lpr)
    return pad.reshape(m, K, lpr, 4), valid


def _fwd_one(x, gamma, beta, res, eps, defect, bf16):
    m, c = x.shape
    v, valid = _fwd_layout(x.astype(F), c)
    src = _fwd_layout(round_bf16(x), c)[0] if defect == "bf16_stats" else None
    mean, rstd = _fwd_stats(v, valid, c, eps, defect, src)
    gm = np.roll(gamma, 1) if defect == "gamma_shift" else gamma
    gm = _fwd_layout(gm.astype(F)[None], c)[0]
    bt = _fwd_layout(beta.astype(F)[None], c)[0]
    with np.errstate(invalid="ignore", over="ignore"):
        y = (v - mean) * rstd * gm + bt
    if res is not None:
        y = y + _fwd_layout(res.astype(F), c)[0]
    y = y.reshape(m, -1)[:, :c].astype(F)
    return round_bf16(y) if bf16 else y


def layernorm_emulated(x, gamma, beta, eps=EPS, res=None, gamma2=None, beta2=None, bf16=False, defect=None):
    """layernorm_kernel in numpy float32: per lane the chunks sub, sub + LPR, ... one after the other, (a + b) + (c + d)
    inside a chunk, a butterfly over the LPR lanes, two-pass variance; the chained norm reads the stored y.
    Returns y or (y, y2)."""
    y = _fwd_one(x, gamma, beta, res, eps, defect, bf16)
    if gamma2 is None:
        return y
    return y, _fwd_one(y, gamma2, beta2, None, eps, defect, bf16)


def _slab_sum_emulated(slab):
    """slab_sum_kernel: lane z adds chunks z, z + 16, ... in order; the 16 lane sums are added in lane order"""
    ns, n = slab.shape
    pad = np.zeros((-(-ns // 16) * 16, n), dtype=F)
    pad[:ns] = slab
    pad = pad.reshape(-1, 16, n)
    s = np.zeros((16, n), dtype=F)
    for i in range(pad.shape[0]):
        s = s + pad[i]
    t = np.zeros(n, dtype=F)
    for z in range(16):
        t = t + s[z]
    return t


def _col_sums_emulated(p, c, variant):
    """column sums of p (m, c) float32 in the order of the backward kernels: per row chunk, per wave / partial row slot,
    then across them, then the slab sum"""
    m = p.shape[0]
    rb, ns = row_chunks(m)
    parts = 1024 // c if variant == "packed" else 4
    steps = -(-rb // parts)
    pad = np.zeros((ns, steps * parts, c), dtype=F)
    flat = np.zeros((ns * rb, c), dtype=F)
    flat[:m] = p
    pad[:, :rb] = flat.reshape(ns, rb, c)
    pad = pad.reshape(ns, steps, parts, c)
    acc = np.zeros((ns, parts, c), dtype=F)
    for i in range(steps):
        acc = acc + pad[:, i]
    if variant == "packed":
        slab = np.zeros((ns, c), dtype=F)
        for q in range(parts):
            slab = slab + acc[:, q]
    else:
        slab = (acc[:, 0] + acc[:, 1]) + (acc[:, 2] + acc[:, 3])
    return _slab_sum_emulated(slab)


def layernorm_bwd_emulated(x, dy, gamma, eps=EPS, add=None, bf16=False, defect=None):
    """layernorm_bwd_kernel<NC> / layernorm_bwd_packed_kernel in numpy float32 -> dx, dgamma, dbeta"""
    m, c = x.shape
    variant = backward_variant(c)
    if variant == "packed":
        lanes, per = c // 4, 4                          # lane gl owns columns 4 gl .. 4 gl + 3
        lay = lambda a: a.astype(F).reshape(a.shape[0], lanes, per)
        unlay = lambda a: a.reshape(a.shape[0], c)
    else:
        lanes, per = 64, variant                        # lane owns columns lane, lane + 64, ...
        def lay(a):
            pad = np.zeros((a.shape[0], per * 64), dtype=F)
            pad[:, :c] = a
            return pad.reshape(a.shape[0], per, 64).transpose(0, 2, 1)
        unlay = lambda a: a.transpose(0, 2, 1).reshape(a.shape[0], per * 64)[:, :c]
    valid = lay(np.ones((1, c), dtype=F)) > 0
    xv, dv = lay(x), lay(dy)
    gm = lay((np.roll(gamma, 1) if defect == "gamma_shift" else gamma)[None])
    inv_c = F(1.0) / F(c + 1 if defect == "cplus1" else c)

    def lane_sum(t):                                   # (m, lanes, per) -> (m, 1, 1)
        if variant == "packed":
            s = (t[..., 0] + t[..., 1]) + (t[..., 2] + t[..., 3])
        else:
            s = np.zeros(t.shape[:2], dtype=F)
            for k in range(per):
                s = s + t[..., k]
        return _butterfly(s)[:, :, None]

    def lane_chain(t):                                 # q, s1, s2: one element after the other in both kernels
        s = np.zeros(t.shape[:2], dtype=F)
        for k in range(per):
            s = s + t[..., k]
        return _butterfly(s)[:, :, None]

    mean = lane_sum(xv) * inv_c
    d = np.where(valid, xv - mean, F(0))
    var = lane_chain(d * d) * inv_c
    rstd = _rsqrt(var if defect == "no_eps" else var + F(eps))
    with np.errstate(invalid="ignore", over="ignore"):
        xhat = np.where(valid, d * rstd, F(0))
        g = gm * dv
        s1 = lane_chain(g) * inv_c
        s2 = lane_chain(g * xhat) * inv_c
        if defect == "no_s2":
            s2 = np.zeros_like(s2)
        dx = rstd * (g - s1 - xhat * s2)
        if add is not None:
            a = lay(add)
            dx = a + dx
            if defect == "add_twice":
                dx = dx + a
        dx = unlay(dx).astype(F)
        dg = _col_sums_emulated(unlay(dv * xhat).astype(F), c, variant)
    db = _col_sums_emulated(unlay(dv).astype(F), c, variant)
    return (round_bf16(dx) if bf16 else dx), dg, db


# ------------------------------------------------------------------------------------------------
# GELU
# ------------------------------------------------------------------------------------------------
def gelu_f64(x):
    """x Phi(x) = x erfc(-x / sqrt 2) / 2 (erfc: no cancellation in the negative tail), float64"""
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64))
    return (0.5 * t * torch.special.erfc(-t / math.sqrt(2.0))).numpy()


def gelu_pdf_term_f64(x):
    """x phi(x), float64"""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(under="ignore", over="ignore", invalid="ignore"):
        e = np.exp(-0.5 * np.minimum(x * x, 1e6))
        return x * e / math.sqrt(2.0 * math.pi)


def gelu_grad_f64(x):
    """Phi(x) + x phi(x), float64"""
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64))
    return (0.5 * torch.special.erfc(-t / math.sqrt(2.0))).numpy() + gelu_pdf_term_f64(x)


def bf16_values():
    """every finite bf16 value as float32: 65 280 values, in bit-pattern order"""
    bits = np.arange(1 << 16, dtype=np.uint32)
    bits = bits[(bits & 0x7F80) != 0x7F80]
    return (bits << 16).view(np.float32)


DENSE_POINTS = 196608


def gelu_grid():
    """bf16_values() followed by DENSE_POINTS evenly spaced fp32 values on [-12, 12]: 261 888 = 2046 * 128 values"""
    dense = np.linspace(-12.0, 12.0, DENSE_POINTS).astype(np.float32)
    return np.concatenate([bf16_values(), dense])
