"""CPU statements of the fused AdamW step, its weight shadows and the gradient norm for the kernel tests of
csrc/optim.hip / ptv3_hip/optim.py (no GPU import, nothing from ptv3_hip):

- f32 / HYPERS: the hyperparameter families, and the fp32 rounding ptv3_adamw_step receives them in;
- adamw_step_f64: ONE step in float64 from the fp32 (p, g, m, v) the code under test held before that step, together
  with the per-element bounds E_p, E_m, E_v (derivation below).  A one-step reference: the bound stays a per-step
  rounding bound and does not grow with the step number;
- adamw_step_emulated: the kernel's arithmetic in numpy float32 in its operation order, with or without fused
  multiply-adds, with the host's (double) or the lag branch's (in-kernel fp32) bias corrections and with optional seeded
  defects (DEFECTS): the yardstick that shows E is a bound and is not slack;
- shadow_nat / shadow_t / transpose_index: the weight shadows, bit for bit;
- grad_norm_f64 / grad_norm_bound / grad_norm_emulated: the two-stage sum of squares;
- table_* / layout / make_params / make_grads: seeded input builders (shape sets, gradient families), bf16_edge_values.

The operation (what the C entry point is given: lr, wd, beta1, beta2, eps, grad_scale are fp32 numbers; bc1 = 1 - beta1^t,
bc2 = 1 - beta2^t with t the tensor's OWN step count):
    g' = g * grad_scale
    p1 = p * (1 - lr * wd)
    m' = b1 * m + (1 - b1) * g'
    v' = b2 * v + (1 - b2) * g'^2
    p' = p1 - (lr / bc1) * m' / (sqrt(v') / sqrt(bc2) + eps)

The error bound.  u = 2^-24 (half an fp32 ulp, relative).  p, g, m, v and the hyperparameters are exact fp32 numbers, every
operation is one rounded fp32 operation, |fl(x) - x| <= u |x|, terms of order u^2 are dropped.  A multiply-add may be
fused (one rounding of the sum) or not (product and sum rounded): the unfused form is charged, it has one rounding more.
Division and square root are charged one u (correctly rounded, the compiler's default for fp32 in HIP).
 1. g' = fl(g gs): u |g'|.  c1 = fl(1 - b1), c2 = fl(1 - b2): one u each (exact for b >= 1/2, charged all the same).
 2. m' = fl(fl(b1 m) + fl(c1 g')): the first product u |b1 m|; the second carries c1, g' and its own rounding, 3 u |c1 g'|;
    the sum u |m'|:
      E_m = u (|b1 m| + 3 |c1 g'| + |m'|)
 3. v' = fl(fl(b2 v) + fl(fl(c2 g') g')): c2, g' twice, two products: 5 u |c2 g'^2|:
      E_v = u (|b2 v| + 5 |c2 g'^2| + |v'|)
 4. s = sqrt(v'):  e_s = E_v / (2 s) + u s  (0 where v' = 0: then g' = 0 and v = 0 and every term is exact).
    r = 1 / sqrt(bc2) arrives correctly rounded from double: one u.  den = fl(fl(s r) + eps):
      e_den = r e_s + 2 u s r + u den
 5. q = m' / den:  e_q = E_m / den + |q| e_den / den + u |q|.
 6. step = fl(lr / fl(bc1)), bc1 correctly rounded from double: 2 u relative.  upd = fl(step q):
      e_upd = |step| e_q + 3 u |upd|
 7. decay = fl(1 - fl(lr wd)): e_decay = u (|lr wd| + |decay|);  p1 = fl(p decay): |p| e_decay + u |p1|;  p' = fl(p1 - upd):
      E_p = |p| e_decay + u |p1| + |step| e_q + 3 u |upd| + u |p'|
The same E is asked of the step-lag branch (a tensor whose own count differs from the launch's): its bias corrections are
computed inside the kernel, and have to be about as good as the host's for that.

The gradient norm.  S = sum g^2 over all tensors; a block covers 4096 elements with 256 threads.  A thread adds its 16
squares one after the other (product: 1 u, 15 additions), the block adds its 256 thread sums by an 8-level tree, the
second stage's 256 threads add ceil(blocks / 256) block sums each one after the other and an 8-level tree follows.  All
terms are >= 0, so every rounding is relative to (a part of) S:
      |S32 - S| <= (1 + 15 + 8 + ceil(blocks / 256) + 8) u S
and the square root halves the relative error and adds its own rounding:
      E_norm = norm * u * ((32 + ceil(blocks / 256)) / 2 + 1)"""
import math

import numpy as np
import torch

U = 2.0 ** -24
F = np.float32
CHUNK = 4096                     # elements per block of adamw_kernel / grad_sq_kernel
PTRS = 256                       # gradient pointers per launch
TINY = 1e-300


def f32(x):
    """the fp32 number a C float argument receives"""
    return float(np.float32(x))


def _f64(a):
    """float64 of a numpy array, a torch tensor or a number (the reference and the bounds use operators, abs() and **
    only, so they run on either; the GPU tests evaluate them in torch float64 on the device)"""
    if isinstance(a, torch.Tensor):
        return a.double()
    return np.asarray(a, dtype=np.float64)


# ------------------------------------------------------------------------------------------------
# hyperparameter families
# ------------------------------------------------------------------------------------------------
# lr / wd: one value per parameter group (two groups; the fork config: "block" parameters at a tenth of the rate)
HYPERS = {
    "fork":      dict(lr=(2e-3, 2e-4), wd=(5e-3, 5e-3), betas=(0.9, 0.999), eps=1e-8, gs=1.0),
    "fork_clip": dict(lr=(2e-3, 2e-4), wd=(5e-3, 5e-3), betas=(0.9, 0.999), eps=1e-8, gs=0.37),
    # the update is comparable with |p|: a relative step-size error of 1e-6 shows in p (at lr = 1e-3 it hides behind u |p|)
    "half":      dict(lr=(0.5, 0.5), wd=(5e-3, 0.0), betas=(0.9, 0.999), eps=1e-8, gs=1.0),
    "half_b99":  dict(lr=(0.5, 0.25), wd=(1e-2, 5e-3), betas=(0.9, 0.99), eps=1e-8, gs=0.37),
    "nowd":      dict(lr=(1e-3, 1e-3), wd=(0.0, 0.0), betas=(0.9, 0.99), eps=1e-8, gs=1.0),
}
GRAD_FAMILIES = ("normal", "tiny", "large", "zero", "mixed")
DEFECTS = ("eps_before_bc2", "decay_after", "bc2_prev_step", "scale_g_not_g2")


def bias_corrections(b1, b2, step):
    """1 - beta^step in float64 from the fp32 betas; step: a number, a numpy array or a torch tensor"""
    return 1.0 - b1 ** step, 1.0 - b2 ** step


def adamw_step_f64(p, g, m, v, lr, wd, b1, b2, eps, gs, step):
    """One step in float64 and its bounds: dict(p, m, v, E_p, E_m, E_v).  lr, wd, step: numbers or per-element arrays;
    every hyperparameter must already be an fp32 number (f32())."""
    p, g, m, v = _f64(p), _f64(g), _f64(m), _f64(v)
    gp = g * gs
    decay = 1.0 - lr * wd
    p1 = p * decay
    c1, c2 = 1.0 - b1, 1.0 - b2
    m1 = b1 * m + c1 * gp
    v1 = b2 * v + c2 * gp * gp
    bc1, bc2 = bias_corrections(b1, b2, step)
    r = bc2 ** -0.5
    s = v1 ** 0.5
    den = s * r + eps
    ss = lr / bc1
    q = m1 / den
    upd = ss * q
    p2 = p1 - upd
    E_m = U * (abs(b1 * m) + 3 * abs(c1 * gp) + abs(m1))
    E_v = U * (abs(b2 * v) + 5 * abs(c2 * gp * gp) + abs(v1))
    e_s = E_v / (2 * s + TINY) + U * s
    e_den = r * e_s + 2 * U * s * r + U * den
    e_q = E_m / den + abs(q) * e_den / den + U * abs(q)
    e_decay = U * (abs(lr * wd) + abs(decay))
    E_p = abs(p) * e_decay + U * abs(p1) + abs(ss) * e_q + 3 * U * abs(upd) + U * abs(p2)
    return dict(p=p2, m=m1, v=v1, E_p=E_p, E_m=E_m, E_v=E_v)


# ------------------------------------------------------------------------------------------------
# fp32 emulation of adamw_kernel
# ------------------------------------------------------------------------------------------------
def _fma(a, b, c):
    """fl(a b + c): the product of two fp32 numbers is exact in float64"""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F)


def _host_bc(b1, b2, step):
    """ptv3_adamw_step: (float)(1 - pow(b1, t)), (float)(1 / sqrt(1 - pow(b2, t))) from double"""
    t = np.asarray(step, np.float64)
    with np.errstate(divide="ignore"):
        return (1.0 - float(b1) ** t).astype(F), (1.0 / np.sqrt(1.0 - float(b2) ** t)).astype(F)


def _lag_bc(b1, b2, step, form):
    """the bias corrections of the step-lag branch, computed in fp32 inside the kernel from the tensor's own count.
    'powf': 1 - powf(beta, own) (powf taken as correctly rounded: the best case) and rsqrtf of it;
    'expm1': -expm1f(own * log_beta) with log_beta rounded from double."""
    own = np.asarray(step, np.float64).astype(F)
    if form == "powf":
        bc1 = F(1) - (np.float64(b1) ** own.astype(np.float64)).astype(F)
        bc2 = F(1) - (np.float64(b2) ** own.astype(np.float64)).astype(F)
    else:
        l1, l2 = F(math.log(float(b1))), F(math.log(float(b2)))
        bc1 = (-np.expm1((own * l1).astype(np.float64))).astype(F)
        bc2 = (-np.expm1((own * l2).astype(np.float64))).astype(F)
    with np.errstate(divide="ignore"):
        return bc1.astype(F), (F(1) / np.sqrt(bc2.astype(F))).astype(F)


def adamw_step_emulated(p, g, m, v, lr, wd, b1, b2, eps, gs, step, fused=True, bc="host", defect=None):
    """adamw_kernel's update in numpy float32 -> (p, m, v).  fused: multiply-adds contracted inside one expression, as
    -ffp-contract=on allows; bc: 'host' (the launch arguments), 'powf' or 'expm1' (the lag branch, _lag_bc)."""
    assert defect is None or defect in DEFECTS
    p, g, m, v = (np.asarray(a, F) for a in (p, g, m, v))
    lr, wd = np.asarray(lr, F), np.asarray(wd, F)
    b1, b2, eps, gs = F(b1), F(b2), F(eps), F(gs)
    t = np.asarray(step, np.float64)
    bc1, r = _host_bc(b1, b2, t) if bc == "host" else _lag_bc(b1, b2, t, bc)
    if defect == "bc2_prev_step":
        r = _host_bc(b1, b2, t - 1)[1]
    one = F(1)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        ss = (lr / bc1).astype(F)
        decay = _fma(-lr, wd, one) if fused else (one - (lr * wd).astype(F)).astype(F)
        c1, c2 = one - b1, one - b2
        g0 = g
        g = (g * gs).astype(F)
        gv = g0 if defect == "scale_g_not_g2" else g
        if defect != "decay_after":
            p = (p * decay).astype(F)
        sq = ((c2 * gv).astype(F) * gv).astype(F)
        if fused:
            m = _fma(b1, m, (c1 * g).astype(F))
            v = _fma(b2, v, sq)
        else:
            m = ((b1 * m).astype(F) + (c1 * g).astype(F)).astype(F)
            v = ((b2 * v).astype(F) + sq).astype(F)
        s = np.sqrt(v).astype(F)
        if defect == "eps_before_bc2":
            den = ((s + eps).astype(F) * r).astype(F)
        else:
            den = _fma(s, r, eps) if fused else ((s * r).astype(F) + eps).astype(F)
        q = (m / den).astype(F)
        p = _fma(-ss, q, p) if fused else (p - (ss * q).astype(F)).astype(F)
        if defect == "decay_after":
            p = (p * decay).astype(F)
    return p, m, v


# ------------------------------------------------------------------------------------------------
# weight shadows
# ------------------------------------------------------------------------------------------------
def weight_dims(shape):
    """(rows, kvol, cols) of a >= 2-d weight: Linear (out, in) -> (out, 1, in), SubMConv3d (out, k, k, k, in)"""
    rows, cols = shape[0], shape[-1]
    return rows, int(np.prod(shape)) // (rows * cols), cols


def transpose_index(rows, kvol, cols):
    """src with t.flat[i] = nat.flat[src[i]]:  t[(c kvol + (kvol - 1 - d)) rows + o] = nat[(o kvol + d) cols + c]"""
    o, d, c = np.meshgrid(np.arange(rows), np.arange(kvol), np.arange(cols), indexing="ij")
    src = np.empty(rows * kvol * cols, dtype=np.int64)
    src[((c * kvol + (kvol - 1 - d)) * rows + o).reshape(-1)] = ((o * kvol + d) * cols + c).reshape(-1)
    return src


def shadow_nat(p, dtype):
    """p (torch, fp32) in the shadow dtype, (rows, kvol * cols)"""
    rows, kvol, cols = weight_dims(tuple(p.shape))
    return p.detach().to(dtype).reshape(rows, kvol * cols)


def shadow_t(p, dtype):
    """the transposed, tap-mirrored shadow (cols, kvol * rows), element by element from the index formula"""
    rows, kvol, cols = weight_dims(tuple(p.shape))
    src = torch.from_numpy(transpose_index(rows, kvol, cols)).to(p.device)
    return shadow_nat(p, dtype).reshape(-1)[src].reshape(cols, kvol * rows)


def shadowed(shape):
    """FusedAdamW._shadow: >= 2-d with rows and cols multiples of 8"""
    return len(shape) >= 2 and shape[0] % 8 == 0 and shape[-1] % 8 == 0


def bf16_edge_values():
    """fp32 values around every rounding decision of fp32 -> bf16, all finite with a finite bf16 image: exact ties between
    two bf16 neighbours with the kept bit even and odd, the fp32 neighbours of those ties, bf16-subnormal magnitudes
    (ties and neighbours among them), +-0, the largest finite bf16 and the largest fp32 below the tie that would round to
    infinity.  Both signs; 512 values (a multiple of 4: the vector path), shuffled by a fixed permutation."""
    bits = []
    for hi in (0x3F80, 0x3F81, 0x4049, 0x4048, 0x0080, 0x0081, 0x7F00, 0x7F01, 0x7F7E,      # normal: even and odd kept bit
               0x0000, 0x0001, 0x0002, 0x0003, 0x007F, 0x007E, 0x0040):                       # bf16 subnormals
        for lo in (0x0000, 0x0001, 0x7FFF, 0x8000, 0x8001, 0xFFFF):
            bits.append((hi << 16) | lo)
    bits += [0x7F7F0000, 0x7F7F0001, 0x7F7F7FFF]           # largest finite bf16; below the tie to infinity
    bits = np.array(bits, dtype=np.uint32)
    bits = np.concatenate([bits, bits | np.uint32(0x80000000)])
    vals = bits.view(np.float32)
    return np.resize(vals, 512)[np.random.default_rng(5).permutation(512)].copy()


# ------------------------------------------------------------------------------------------------
# gradient norm
# ------------------------------------------------------------------------------------------------
def blocks_of(counts):
    return sum(-(-n // CHUNK) for n in counts)


def grad_norm_f64(grads):
    """sqrt(sum of squares) in float64 of a list of numpy arrays"""
    return math.sqrt(sum(float((np.asarray(g, np.float64) ** 2).sum()) for g in grads))


def grad_norm_bound(norm, blocks):
    """E_norm of the module docstring"""
    return norm * U * ((32 + -(-blocks // 256)) / 2 + 1)


def _tree256(red):
    d = 128
    while d > 0:
        red[:d] = red[:d] + red[d:2 * d]
        d >>= 1
    return red[0]


def grad_norm_emulated(grads, fused=True, defect=None):
    """grad_sq_kernel + sum_partials_kernel + sqrt in numpy float32.  defect 'drop_last_partial': the last, partial block
    of a tensor is left out."""
    partial = []
    for g in grads:
        g = np.asarray(g, F).reshape(-1)
        nb = -(-g.size // CHUNK)
        for b in range(nb):
            blk = g[b * CHUNK:(b + 1) * CHUNK]
            if defect == "drop_last_partial" and blk.size < CHUNK:
                partial.append(F(0))
                continue
            pad = np.zeros(CHUNK, dtype=F)
            pad[:blk.size] = blk
            pad = pad.reshape(16, 256)                    # thread t: elements t, t + 256, ...
            s = np.zeros(256, dtype=F)
            for k in range(16):
                s = _fma(pad[k], pad[k], s) if fused else (s + (pad[k] * pad[k]).astype(F)).astype(F)
            partial.append(_tree256(s.copy()))
    if not partial:
        return F(0)
    n = len(partial)
    pad = np.zeros(-(-n // 256) * 256, dtype=F)
    pad[:n] = np.array(partial, dtype=F)
    pad = pad.reshape(-1, 256)
    s = np.zeros(256, dtype=F)
    for k in range(pad.shape[0]):
        s = (s + pad[k]).astype(F)
    return np.sqrt(_tree256(s.copy())).astype(F)


# ------------------------------------------------------------------------------------------------
# shape sets: a table is a list of (numel, parameter offset, gradient offset); an offset of 1 makes that pointer a
# contiguous view one element past a 16-byte boundary (the scalar path for a numel that is a multiple of 4)
# ------------------------------------------------------------------------------------------------
COUNTS = (1, 3, 4, 1020, 1023, 1024, 1025, 4092, 4095, 4096, 4097, 4100, 8192, 12289)
LARGE_TABLES = (257, 512, 513, 600)
EMPTY_PLACES = ("first", "middle", "last", "at255", "at256", "own_run")


def table_counts():
    """every element count, then every count that is a multiple of 4 again with the parameter, the gradient and both
    one element off alignment: 14 + 3 * 7 = 35 tensors"""
    t = [(n, 0, 0) for n in COUNTS]
    for n in COUNTS:
        if n % 4 == 0:
            t += [(n, 1, 0), (n, 0, 1), (n, 1, 1)]
    return t


def table_large(ntensors, seed=0):
    """most tensors hold 1 to 64 elements (fewer than one block's worth: the launch boundaries fall inside series of
    one-block tensors); multi-block tensors sit on both sides of every 256-tensor boundary; a tenth are misaligned views"""
    g = np.random.default_rng([seed, ntensors])
    sizes = g.integers(1, 65, ntensors)
    off = g.random((ntensors, 2)) < 0.1
    multi = {3: 4097, 254: 4097, 255: 8192, 256: 4096, 257: 12289, 300: 5000,
             510: 8192, 511: 4100, 512: 4097, 513: 8195, 599: 4097}
    t = []
    for i in range(ntensors):
        n = multi.get(i, int(sizes[i]))
        if i == ntensors - 1 and ntensors in (257, 513):
            n = 4097                                        # the run that holds one tensor only has two blocks
        t.append((n, int(off[i, 0]), int(off[i, 1])))
    return t


def table_with_empty(place):
    """a zero-element tensor first, in the middle and last of a short table, at table positions 255 and 256, and as the
    only tensor of the third launch of a 513-tensor table (a run without blocks)"""
    short = [(5, 0, 0), (4096, 0, 0), (64, 0, 0), (1025, 0, 0), (8192, 0, 1), (3, 0, 0)]
    if place == "first":
        return [(0, 0, 0)] + short
    if place == "middle":
        return short[:2] + [(0, 0, 0)] + short[2:4] + [(0, 0, 0), (0, 0, 0)] + short[4:]
    if place == "last":
        return short + [(0, 0, 0)]
    if place in ("at255", "at256"):
        t = table_large(300, seed=1)
        t[int(place[2:])] = (0, 0, 0)
        return t
    assert place == "own_run"
    t = table_large(513, seed=2)
    t[512] = (0, 0, 0)
    return t


GAP = 8             # guard elements around every tensor of a flat buffer


def layout(table, which):
    """element offsets of the tensors in one flat buffer (which: 0 parameters, 1 gradients) and its length: each tensor
    starts GAP or more elements after the previous one, at a multiple of 4 plus its offset"""
    offs, at = [], GAP
    for spec in table:
        at = -(-at // 4) * 4 + spec[1 + which]
        offs.append(at)
        at += spec[0] + GAP
    return offs, at + GAP


def grad_scales(table, family, seed=0):
    """the gradient scale of every tensor of the table"""
    assert family in GRAD_FAMILIES
    if family == "mixed":
        return 10.0 ** np.random.default_rng([seed, len(table), 77]).uniform(-4.0, 3.0, len(table))
    return np.full(len(table), dict(normal=1.0, tiny=1e-4, large=1e3, zero=0.0)[family])


def make_params(table, seed):
    """the flat parameter buffer (float32, guards = CANARY) and the tensors' offsets"""
    offs, total = layout(table, 0)
    buf = np.full(total, CANARY, dtype=F)
    g = np.random.default_rng([seed, len(table), 1])
    for (n, _, _), o in zip(table, offs):
        buf[o:o + n] = g.standard_normal(n).astype(F)
    return buf, offs


def make_grads(table, family, seed, step):
    """the flat gradient buffer of one step (guards = CANARY) and the tensors' offsets"""
    offs, total = layout(table, 1)
    buf = np.full(total, CANARY, dtype=F)
    g = np.random.default_rng([seed, len(table), 2, step])
    sc = grad_scales(table, family, seed)
    for (n, _, _), o, s in zip(table, offs, sc):
        buf[o:o + n] = (s * g.standard_normal(n)).astype(F)
    return buf, offs


CANARY = F(-768.0)

# weights of the shadow tests as (rows, kvol, cols), and what sits between them
SHADOW_WEIGHTS = ((8, 1, 8), (64, 1, 64), (72, 1, 40), (136, 1, 200), (512, 1, 128), (16, 27, 8), (72, 27, 64), (24, 125, 16))
UNSHADOWED = ((32, 27, 6), (12, 16), (40,), (1025,), (7,))


def shadow_orders():
    """three orders of the same tensors: unshadowed ones first, between and last"""
    w = [s if s[1] > 1 else (s[0], s[2]) for s in SHADOW_WEIGHTS]
    u = list(UNSHADOWED)
    return [u[:3] + w + u[3:],                                                        # first and last
            [w[0], u[0], w[1], w[2], u[1], u[2], w[3], u[3], w[4], w[5], u[4], w[6], w[7]],   # between, shadowed first / last
            u[3:] + w[::-1] + u[:3]]
