"""Swin3D window partition + cRSE window attention on the GPU (row A19) vs oracle/swin3d.py.

PARITY UNPINNED: the reference runs this path in MinkowskiEngine and microsoft/Swin3D, neither of which is in its
tree, and it holds no test, fixture or golden vector for it; the oracle restates swin3d_layers.py's index bookkeeping
and the Swin3D paper's cRSE formula (assumptions listed in its header).  Window partition: exact.  Attention: fp32
relative L2 <= 1e-4 (the north_star's fp32 budget), bf16 storage <= 2e-2."""
import numpy as np
import pytest
import torch

from oracle import swin3d as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X box"
    return torch.device("cuda:0")


def _voxels(n, extent, seed, batch=1, stride=1, lo=0):
    rng = np.random.default_rng(seed)
    c = np.unique(rng.integers(lo, lo + extent, size=(n * 2, 3)), axis=0)
    c = c[rng.permutation(len(c))[:n]]
    b = rng.integers(0, batch, size=(len(c), 1))
    return np.concatenate([b, c * stride], axis=1).astype(np.int32)


def _surface(n, extent, seed):
    """Voxels on a wavy sheet: windows hold a realistic 20-60 of their 125 / 343 cells."""
    rng = np.random.default_rng(seed)
    xy = rng.uniform(0, extent, size=(3 * n, 2))
    z = extent / 2 + extent / 6 * np.sin(xy[:, 0] / 9.0) * np.cos(xy[:, 1] / 7.0) + rng.normal(0, 0.4, 3 * n)
    g = np.unique(np.floor(np.concatenate([xy, z[:, None]], 1)).astype(np.int64), axis=0)
    g = g[rng.permutation(len(g))[:n]]
    return np.concatenate([np.zeros((len(g), 1), np.int64), g], 1).astype(np.int32)


@pytest.mark.parametrize("ws,shift,stride,lo,batch", [(5, 0, 1, 0, 1), (5, 2, 1, 0, 3), (7, 3, 2, -60, 2), (3, 1, 4, -9, 2),
                                                       (8, 4, 1, 0, 1)])
def test_window_mapping_exact(dev, ws, shift, stride, lo, batch):
    from ptv3_hip import ops
    c = _voxels(5000, 48, ws * 10 + shift, batch=batch, stride=stride, lo=lo)
    w_w_id, w_w_xyz, nempty, sort_idx, inv = O.window_mapping(c, stride, ws, shift)
    g = ops.swin_window_mapping(torch.from_numpy(c).to(dev), stride, ws, shift)
    gw_id, gw_xyz, gsizes, gsort, ginv, gstart = (t.cpu().numpy() for t in g)
    assert np.array_equal(gw_id, w_w_id) and np.array_equal(gw_xyz, w_w_xyz)
    assert np.array_equal(gsizes, nempty) and np.array_equal(gsort, sort_idx) and np.array_equal(ginv, inv)
    assert np.array_equal(gstart, np.concatenate([[0], np.cumsum(nempty)]))


def test_window_mapping_rejects_coordinates_outside_the_key(dev):
    from ptv3_hip import ops
    c = np.array([[0, 0, 0, 0], [0, 5 * 5000, 0, 0]], np.int32)
    with pytest.raises(ValueError, match="window coordinate"):
        ops.swin_window_mapping(torch.from_numpy(c).to(dev), 1, 5, 0)
    with pytest.raises(RuntimeError, match="window_size"):
        ops.swin_window_mapping(torch.from_numpy(c).to(dev), 1, 9, 0)


def _case(coords, heads, hd, ws, quant, crse, seed, shift=0, table_std=0.3):
    rng = np.random.default_rng(seed)
    n = len(coords)
    w_w_id, w_w_xyz, nempty, sort_idx, _ = O.window_mapping(coords, 1, ws, shift)
    nsig = {"XYZ": 0, "XYZ_RGB": 3, "XYZ_RGB_NORM": 6}[crse]
    sig = rng.uniform(-1, 1, (n, nsig)).astype(np.float32)
    if nsig:
        sig[:4, :3] = [[-1, -1, -1], [1, 1, 1], [1, -1, 1], [-1, 1, -1]]        # the +-2 differences that need the clamp
    nc = O.n_coords(w_w_xyz, rng.random((n, 3), dtype=np.float32), sig, sort_idx)
    rows = O.table_lengths(ws, quant, crse)
    offs = [r * heads * hd for r in rows for _ in range(3)]
    tabs = [rng.normal(0, table_std, sum(offs)).astype(np.float32) for _ in range(3)]
    q, k, v = (rng.normal(size=(n, heads, hd)).astype(np.float32) for _ in range(3))
    q *= hd ** -0.5
    _, _, _, w_sizes, w2n, _ = O.sparse_self_attention(nempty)
    return q, k, v, tabs, offs, w_sizes, w2n, sort_idx, O.n_crse(nc, quant, crse)


def _run(dev, case, ws, dtype=torch.float32):
    from ptv3_hip import ops
    q, k, v, tabs, offs, w_sizes, w2n, n2n, cr = case
    t = lambda a, d=None: torch.from_numpy(np.ascontiguousarray(a)).to(dev) if d is None else \
        torch.from_numpy(np.ascontiguousarray(a)).to(dev).to(d)
    w_start = np.concatenate([w2n, [len(q)]]).astype(np.int32)
    out = ops.swin_attention(t(q, dtype), t(k, dtype), t(v, dtype), t(tabs[0]), t(tabs[1]), t(tabs[2]), offs,
                             t(n2n.astype(np.int64)), t(w_start), t(cr), ws ** 3)
    torch.cuda.synchronize()
    return out.float().cpu().numpy()


def _rel(a, b):
    return float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-30))


@pytest.mark.parametrize("heads,hd,ws,quant,crse", [(6, 8, 5, 4, "XYZ_RGB_NORM"), (6, 16, 7, 4, "XYZ_RGB_NORM"),
                                                     (4, 16, 5, 50, "XYZ_RGB"), (2, 32, 5, 4, "XYZ"),
                                                     (3, 16, 3, 2, "XYZ_RGB_NORM")])
def test_crse_attention_fp32(dev, heads, hd, ws, quant, crse):
    coords = _surface(4000, 60, heads * 100 + hd)
    case = _case(coords, heads, hd, ws, quant, crse, seed=hd + ws)
    want = O.crse_attention(*case[:3], *case[3], *case[4:])
    got = _run(dev, case, ws)
    assert _rel(got, want) <= 1e-4, _rel(got, want)
    assert np.abs(got - want).max() <= 1e-4 * max(1.0, np.abs(want).max())


def test_crse_attention_dense_windows_and_shift(dev):
    """Fully occupied 7^3 windows (343 tokens: six key chunks per wave, the largest LDS footprint) on the shifted
    partition, plus windows of a single voxel."""
    g = np.stack(np.meshgrid(np.arange(15), np.arange(14), np.arange(12), indexing="ij"), -1).reshape(-1, 3)
    lone = np.array([[200, 200, 200], [300, 10, 50]])
    coords = np.concatenate([np.zeros((len(g) + 2, 1), np.int64), np.concatenate([g, lone])], 1).astype(np.int32)
    case = _case(coords, 2, 16, 7, 4, "XYZ_RGB_NORM", seed=7, shift=3)
    assert case[5].max() == 343 and case[5].min() == 1
    want = O.crse_attention(*case[:3], *case[3], *case[4:])
    got = _run(dev, case, 7)
    assert _rel(got, want) <= 1e-4, _rel(got, want)


@pytest.mark.parametrize("hd", [8, 16, 32])
@pytest.mark.parametrize("crse", ["XYZ", "XYZ_RGB", "XYZ_RGB_NORM"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_crse_attention_matrix_core_kernel_vs_gather_kernel(dev, hd, crse, dtype):
    """swin_attn_mfma_kernel (table products on the matrix core, scalar lookups in LDS: the default for short tables)
    against swin_attn_kernel (row gathers; PTV3_SWIN_ATTN_MFMA=0) on the same inputs, every (head_dim, signal axes)
    instantiation, windows of 1 .. 60 tokens (one to four query tiles, ragged last tiles), then against the oracle."""
    import os
    coords = _surface(2500, 40, hd)
    case = _case(coords, 3, hd, 5, 4, crse, seed=hd)
    assert case[5].min() < 16 < 33 < case[5].max()
    got = _run(dev, case, 5, dtype)
    os.environ["PTV3_SWIN_ATTN_MFMA"] = "0"
    try:
        gather = _run(dev, case, 5, dtype)
    finally:
        os.environ.pop("PTV3_SWIN_ATTN_MFMA", None)
    tol = 2e-5 if dtype == torch.float32 else 2.0 ** -7      # fp32: summation order only; bf16: one output rounding
    assert np.abs(got - gather).max() <= tol * max(1.0, np.abs(gather).max())
    if dtype == torch.float32:
        assert not np.array_equal(got, gather)                  # two kernels did run (different summation order)
        want = O.crse_attention(*case[:3], *case[3], *case[4:])
        assert _rel(got, want) <= 1e-4, _rel(got, want)


def test_crse_attention_bf16_storage(dev):
    coords = _surface(3000, 50, 5)
    case = _case(coords, 6, 16, 5, 4, "XYZ_RGB_NORM", seed=11)
    rb = lambda a: torch.from_numpy(a).bfloat16().float().numpy()
    want = O.crse_attention(rb(case[0]), rb(case[1]), rb(case[2]), *case[3], *case[4:])
    got = _run(dev, case, 5, torch.bfloat16)
    assert _rel(got, want) <= 1e-2, _rel(got, want)       # one bf16 rounding of the output


def test_crse_attention_argument_checks(dev):
    from ptv3_hip import ops
    coords = _surface(500, 30, 1)
    case = _case(coords, 3, 12, 5, 4, "XYZ", seed=1)
    with pytest.raises(RuntimeError, match="head_dim"):
        _run(dev, case, 5)
    case = _case(coords, 3, 16, 5, 4, "XYZ", seed=1)
    q, k, v, tabs, offs, w_sizes, w2n, n2n, cr = case
    with pytest.raises(RuntimeError, match="table_offsets"):
        _run(dev, (q, k, v, tabs, [o - 16 for o in offs], w_sizes, w2n, n2n, cr), 5)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        ops.swin_attention(torch.zeros(4, 3, 16), torch.zeros(4, 3, 16), torch.zeros(4, 3, 16), torch.zeros(8),
                           torch.zeros(8), torch.zeros(8), offs, torch.zeros(4, dtype=torch.int64),
                           torch.zeros(2, dtype=torch.int32), torch.zeros(4, 3), 125)


def _np_ln(x, g, b, eps=1e-5):
    mu = x.mean(-1, keepdims=True)
    var = ((x - mu) ** 2).mean(-1, keepdims=True)
    return (x - mu) / np.sqrt(var + eps) * g + b


def _np_gelu(x):
    from scipy.special import erf
    return 0.5 * x * (1.0 + erf(x / np.sqrt(2.0)))


def test_window_stage_two_blocks_regular_then_shifted(dev):
    """WindowStage = the block loop of BasicLayer (swin3d_layers.py:846-866): block 0 on the regular partition,
    block 1 on the half-window shift, each LN -> cRSE attention -> proj -> residual -> LN -> MLP -> residual
    (:619-630), against the same composition of oracle pieces in float64 / fp32."""
    from pointcept.models.swin3d import WindowStage
    torch.manual_seed(3)
    dim, heads, ws, quant, crse = 48, 6, 5, 4, "XYZ_RGB_NORM"
    stage = WindowStage(dim, 2, heads, ws, quant, cRSE=crse)
    with torch.no_grad():
        for name, p in stage.named_parameters():
            if name.endswith("_table"):
                p.normal_(0, 0.2)                     # the 0.02 initialisation would hide an indexing error
            elif name.endswith("norm1.weight") or name.endswith("norm2.weight"):
                p.uniform_(0.5, 1.5)
            elif name.endswith("bias"):
                p.normal_(0, 0.1)
    stage = stage.to(dev).eval()
    coords = _surface(3000, 50, 9)
    n = len(coords)
    rng = np.random.default_rng(0)
    local = rng.random((n, 3), dtype=np.float32)
    sig = rng.uniform(-1, 1, (n, 6)).astype(np.float32)
    feats = rng.normal(size=(n, dim)).astype(np.float32)
    with torch.no_grad():
        got = stage(torch.from_numpy(feats).to(dev), torch.from_numpy(coords).to(dev), 1,
                    torch.from_numpy(local).to(dev), torch.from_numpy(sig).to(dev)).cpu().numpy()
    sd = {k: v.detach().cpu().numpy() for k, v in stage.state_dict().items()}
    x = feats.astype(np.float64)
    for i, shift in enumerate((0, ws // 2)):
        pre = f"blocks.{i}."
        w_w_id, w_w_xyz, nempty, sort_idx, _ = O.window_mapping(coords, 1, ws, shift)
        nc = O.n_coords(w_w_xyz, local, sig, sort_idx)
        args = (*O.sparse_self_attention(nempty)[:3], nempty, O.sparse_self_attention(nempty)[4], sort_idx, None, nc)
        params = {k[len(pre) + 5:]: v for k, v in sd.items() if k.startswith(pre + "attn.")}
        h = _np_ln(x, sd[pre + "norm1.weight"], sd[pre + "norm1.bias"]).astype(np.float32)
        x = x + O.window_attention_forward(params, h, args, heads, quant, crse)
        h = _np_ln(x, sd[pre + "norm2.weight"], sd[pre + "norm2.bias"])
        h = _np_gelu(h @ sd[pre + "mlp.fc1.weight"].T.astype(np.float64) + sd[pre + "mlp.fc1.bias"])
        x = x + h @ sd[pre + "mlp.fc2.weight"].T.astype(np.float64) + sd[pre + "mlp.fc2.bias"]
    assert _rel(got, x) <= 1e-4, _rel(got, x)


# ---------------------------------------------------------------------------------------------------------------
# whole model
# ---------------------------------------------------------------------------------------------------------------
def _swin_batch(sizes, seed, sig_dim=6, feat_dim=9, grid=0.02, dup=0.15):
    """Scenes on wavy sheets.  coord = (voxel + sub-voxel offset) * grid, so coord / base_grid_size - grid_coord is the
    sub-voxel offset the cRSE expects; `dup` of the voxels hold two points (voxel averaging, :162-181)."""
    rng = np.random.default_rng(seed)
    coords, grids, feats, sigs, offs = [], [], [], [], []
    total = 0
    for b, n in enumerate(sizes):
        g = _surface(n, 46, seed * 10 + b)[:, 1:].astype(np.int64)
        extra = g[rng.random(len(g)) < dup]
        g = np.concatenate([g, extra])
        g = g[rng.permutation(len(g))]
        p = (g + rng.random(g.shape)) * grid
        s = rng.uniform(-1, 1, (len(g), sig_dim))
        grids.append(g)
        coords.append(p)
        sigs.append(s)
        feats.append(rng.normal(size=(len(g), feat_dim)))
        total += len(g)
        offs.append(total)
    return {"coord": np.concatenate(coords).astype(np.float32), "grid_coord": np.concatenate(grids),
            "feat": np.concatenate(feats).astype(np.float32), "coord_feat": np.concatenate(sigs).astype(np.float32),
            "offset": np.asarray(offs, np.int64)}


def _randomise(model, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if name.endswith("_table"):
                p.copy_(torch.randn(p.shape, generator=g) * 0.2)
            elif name.endswith("kernel"):
                p.copy_(torch.randn(p.shape, generator=g) * (1.0 / (p.shape[0] * p.shape[1])) ** 0.5)
            elif p.dim() == 2:
                p.copy_(torch.randn(p.shape, generator=g) * (1.0 / p.shape[1]) ** 0.5)
            elif name.endswith("bias"):
                p.copy_(torch.randn(p.shape, generator=g) * 0.1)
            else:
                p.copy_(torch.rand(p.shape, generator=g) + 0.5)
        for name, b in model.named_buffers():
            if name.endswith("running_mean"):
                b.copy_(torch.randn(b.shape, generator=g) * 0.1)
            elif name.endswith("running_var"):
                b.copy_(torch.rand(b.shape, generator=g) + 0.5)


def _to_dev(batch, dev):
    return {k: torch.from_numpy(v).to(dev) for k, v in batch.items()}


@pytest.mark.parametrize("upsample", ["linear_attn", "linear"])
def test_swin3d_unet_forward_matches_the_restated_model(dev, upsample):
    """"Swin3D-v1m1" end to end (voxel averaging, stem convolution, regular / shifted cRSE attention stages, KNN
    downsampling with the nearest-to-mean signal carrier, 3-NN upsampling with and without its attention block,
    classifier, slice back to the points) against oracle/swin3d.py's Swin3DOracle.  PARITY UNPINNED (see the oracle)."""
    from ptv3_hip import configs
    from pointcept.models import build_model
    cfg = dict(configs.TINY_SWIN3D_CFG, upsample=upsample)
    model = build_model(cfg)
    _randomise(model, 5)
    batch = _swin_batch([2600, 1500], seed=3)
    oracle = O.Swin3DOracle({k: v.numpy() for k, v in model.state_dict().items()}, cfg)
    want = oracle.forward(batch)
    model = model.to(dev).eval()
    with torch.no_grad():
        got = model(_to_dev(batch, dev)).float().cpu().numpy()
    assert got.shape == want.shape == (len(batch["coord"]), 13)
    assert _rel(got, want) <= 1e-4, _rel(got, want)
    # two points of one voxel receive the same row (sp.slice(in_field))
    key = np.concatenate([np.repeat(np.arange(2), np.diff(np.concatenate([[0], batch["offset"]])))[:, None],
                          batch["grid_coord"]], 1)
    _, inv, cnt = np.unique(key, axis=0, return_inverse=True, return_counts=True)
    twin = np.nonzero(cnt[inv.reshape(-1)] > 1)[0]
    assert len(twin) > 100
    first = {}
    for i in twin:
        j = first.setdefault(int(inv.reshape(-1)[i]), i)
        assert np.array_equal(got[i], got[j])


@pytest.mark.parametrize("variant", [dict(knn_down=False), dict(stem_transformer=False),
                                     dict(knn_down=False, stem_transformer=False)])
def test_swin3d_constructor_variants_vs_the_restated_model(dev, variant):
    """GridDownsample (swin3d_layers.py:246-272) and the MinkResBlock stem with its own downsample in front of stage 1
    (swin3d_v1m1_base.py:69-85, 213-216) against the restated model, eval; then one training step runs and every
    parameter receives a finite gradient."""
    from ptv3_hip import configs
    from pointcept.models import build_model
    cfg = dict(configs.TINY_SWIN3D_CFG, **variant)
    model = build_model(cfg)
    _randomise(model, 21)
    batch = _swin_batch([2400, 1700], seed=23)
    oracle = O.Swin3DOracle({k: v.numpy() for k, v in model.state_dict().items()}, cfg)
    want = oracle.forward(batch)
    model = model.to(dev).eval()
    with torch.no_grad():
        got = model(_to_dev(batch, dev)).float().cpu().numpy()
    assert got.shape == want.shape and _rel(got, want) <= 1e-4, _rel(got, want)
    model.train()
    model(_to_dev(batch, dev)).float().square().mean().backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in model.parameters())


def test_swin3d_s3dis_config_end_to_end_vs_the_restated_model(dev):
    """BASELINE configs[4]'s model - Swin3D-S exactly as configs/s3dis/semseg-swin3d-v1m1-0-small.py:12-30 builds it
    (5 levels, depths 2/4/9/4/4, 48..384 channels, 6..24 heads of 8 / 16 channels, 5^3 and 7^3 windows, down_stride 3,
    XYZ_RGB_NORM signals, 28.2 M parameters) - on four scenes (> 20 000 points) against oracle/swin3d.py, fp32 <= 1e-4.
    PARITY UNPINNED (MinkowskiEngine / microsoft Swin3D are not in the reference tree; see the oracle's header)."""
    from ptv3_hip import configs
    from pointcept.models import build_model
    cfg = dict(configs.SWIN3D_S3DIS_CFG)
    model = build_model(cfg)
    assert sum(p.numel() for p in model.parameters()) > 28e6
    _randomise(model, 15)
    batch = _swin_batch([6000, 6000, 6000, 6000], seed=13)
    assert len(batch["coord"]) > 20000
    oracle = O.Swin3DOracle({k: v.numpy() for k, v in model.state_dict().items()}, cfg)
    want = oracle.forward(batch)
    model = model.to(dev).eval()
    with torch.no_grad():
        got = model(_to_dev(batch, dev)).float().cpu().numpy()
    assert got.shape == want.shape == (len(batch["coord"]), 13)
    assert _rel(got, want) <= 1e-4, _rel(got, want)


def test_swin3d_bf16_compute_dtype_close_to_fp32(dev):
    """`model.compute_dtype = torch.bfloat16` (the reference's S3DIS configs run under enable_amp = True): features,
    GEMM / conv operands and q, k, v in bf16, everything that indexes a table or a neighbour in fp32.  Against the fp32
    run of the same weights: logits within a few bf16 steps of the logit scale over the ~60 layers, same class for
    nearly every point."""
    from ptv3_hip import configs
    from pointcept.models import build_model
    model = build_model(dict(configs.SWIN3D_S3DIS_CFG))
    _randomise(model, 15)
    batch = _to_dev(_swin_batch([5000, 4000], seed=3), dev)
    model = model.to(dev).eval()
    with torch.no_grad():
        ref = model(dict(batch))
        model.compute_dtype = torch.bfloat16
        got = model(dict(batch))
    assert got.dtype == torch.float32 and got.shape == ref.shape
    scale = ref.abs().max().item()
    assert (got - ref).abs().max().item() <= 0.08 * scale, ((got - ref).abs().max().item(), scale)
    assert (got - ref).abs().mean().item() <= 0.01 * scale
    assert (got.argmax(1) == ref.argmax(1)).float().mean().item() >= 0.97


def test_offset_keypoint_swin3d_fork_config_vs_the_restated_model(dev):
    """"OffsetKeypointSwin3D" with the fork's own config (configs/my_dataset/offset_keypoint_swin3d.py:14-38: 4 levels
    64..512 channels, 4..32 heads of 16, quant 50, XYZ_RGB, hidden 256) against the restated backbone + a numpy head."""
    from ptv3_hip import configs
    from pointcept.models import build_model
    cfg = dict(configs.OFFSET_SWIN3D_CFG)
    model = build_model(cfg)
    _randomise(model, 19)
    batch = _swin_batch([5000, 4000], seed=16, sig_dim=4, feat_dim=4, dup=0.0)
    batch["feat"] = np.clip(batch.pop("coord_feat"), -1, 1)
    sd = {k: v.numpy() for k, v in model.state_dict().items()}
    oracle = O.Swin3DOracle({k[len("backbone."):]: v for k, v in sd.items() if k.startswith("backbone.")},
                            cfg["backbone_conf"])
    f = oracle.forward(dict(batch, coord_feat=batch["feat"])).astype(np.float64)
    h = f @ sd["head.0.weight"].T + sd["head.0.bias"]
    h = (h - sd["head.1.running_mean"]) / np.sqrt(sd["head.1.running_var"] + 1e-5) * sd["head.1.weight"] + sd["head.1.bias"]
    want = (np.maximum(h, 0) @ sd["head.3.weight"].T + sd["head.3.bias"]).reshape(-1, 6, 4)
    want[..., 3] = 1 / (1 + np.exp(-want[..., 3]))
    model = model.to(dev).eval()
    with torch.no_grad():
        got = model(_to_dev(batch, dev))["pred"].cpu().numpy()
    assert _rel(got, want) <= 1e-4, _rel(got, want)


def test_offset_keypoint_swin3d_wrapper(dev):
    """The fork's wrapper (offset_keypoint_swin3d.py): coord_feat derived from feat, XYZ_RGB cRSE over a 4-channel
    signal (normals + curvature: the attention reads the first three), head + sigmoid on the score, loss when the
    batch carries a target."""
    from pointcept.models import build_model
    cfg = dict(type="OffsetKeypointSwin3D", num_keypoints=6, hidden_dim=32,
               backbone_conf=dict(type="Swin3D-v1m1", in_channels=4, num_classes=32, base_grid_size=0.02, quant_size=50,
                                  num_layers=3, depths=[2, 2, 2], channels=[32, 32, 64], num_heads=[2, 2, 4],
                                  window_sizes=[5, 7, 7], up_k=3, drop_path_rate=0.2, stem_transformer=True,
                                  down_stride=2, upsample="linear", knn_down=True, cRSE="XYZ_RGB", fp16_mode=1))
    model = build_model(cfg)
    _randomise(model, 9)
    batch = _swin_batch([2200, 1800], seed=6, sig_dim=4, feat_dim=4, dup=0.0)
    batch["feat"] = np.clip(batch.pop("coord_feat"), -1, 1)          # the wrapper builds coord_feat from feat
    sd = {k: v.numpy() for k, v in model.state_dict().items()}
    oracle = O.Swin3DOracle({k[len("backbone."):]: v for k, v in sd.items() if k.startswith("backbone.")},
                            cfg["backbone_conf"])
    f = oracle.forward(dict(batch, coord_feat=batch["feat"])).astype(np.float64)
    h = f @ sd["head.0.weight"].T + sd["head.0.bias"]
    h = (h - sd["head.1.running_mean"]) / np.sqrt(sd["head.1.running_var"] + 1e-5) * sd["head.1.weight"] + sd["head.1.bias"]
    want = (np.maximum(h, 0) @ sd["head.3.weight"].T + sd["head.3.bias"]).reshape(-1, 6, 4)
    want[..., 3] = 1 / (1 + np.exp(-want[..., 3]))
    rng = np.random.default_rng(0)
    target = np.concatenate([rng.normal(size=(len(f), 6, 3)), (rng.random((len(f), 6, 1)) > 0.5)], -1).astype(np.float32)
    model = model.to(dev).eval()
    data = _to_dev(batch, dev)
    data["target"] = torch.from_numpy(target).to(dev)
    with torch.no_grad():
        out = model(data)
    got = out["pred"].cpu().numpy()
    assert _rel(got, want) <= 1e-4, _rel(got, want)
    assert "coord_feat" in data and torch.isfinite(out["loss"])


# ---------------------------------------------------------------------------------------------------------------
# backward of the cRSE attention
# ---------------------------------------------------------------------------------------------------------------
def _crse_attention_torch(q, k, v, qt, kt, vt, offs, w_sizes, w2n, n2n, cr):
    """Differentiable torch (float64, CPU) restatement of oracle.swin3d.crse_attention: the checker of the HIP backward
    (torch autograd over the forward this package computes; the reference's own backward lives in the absent
    microsoft/Swin3D: parity unpinned)."""
    n, h, d = q.shape
    starts = np.concatenate([[0], np.cumsum(offs)])
    outs, rows_all = [], []
    for w in range(len(w_sizes)):
        m, s0 = int(w_sizes[w]), int(w2n[w])
        rows = torch.as_tensor(np.asarray(n2n[s0:s0 + m], np.int64))
        c = cr[s0:s0 + m]
        Q, K, V = q[rows], k[rows], v[rows]
        logit = torch.einsum("ihd,jhd->hij", Q, K)
        vsum = 0
        for a in range(len(offs)):
            nrow = int(offs[a]) // (h * d)
            sl = slice(int(starts[a]), int(starts[a + 1]))
            idx = np.floor((c[:, None, a] - c[None, :, a]) + np.float32(nrow // 2)).astype(np.int64).clip(0, nrow - 1)
            idx = torch.from_numpy(idx)
            tq, tk, tv = (t[sl].view(nrow, h, d)[idx] for t in (qt, kt, vt))
            logit = logit + torch.einsum("ihd,ijhd->hij", Q, tk) + torch.einsum("jhd,ijhd->hij", K, tq)
            vsum = vsum + tv
        p = torch.softmax(logit, -1)
        outs.append(torch.einsum("hij,jhd->ihd", p, V) + torch.einsum("hij,ijhd->ihd", p, vsum))
        rows_all.append(rows)
    out = torch.zeros_like(q)
    return out.index_put((torch.cat(rows_all),), torch.cat(outs))


@pytest.mark.parametrize("heads,hd,ws,quant,crse", [(3, 8, 5, 4, "XYZ_RGB_NORM"), (2, 16, 7, 4, "XYZ_RGB"),
                                                     (2, 16, 5, 50, "XYZ_RGB"), (2, 32, 5, 4, "XYZ")])
def test_crse_attention_backward_vs_torch_autograd(dev, heads, hd, ws, quant, crse):
    """ptv3_swin_attn_bwd: dq, dk, dv and the three table gradients against torch autograd (float64) over the restated
    forward, relative L2 <= 1e-4 each.  The fork's table setting (quant 50, XYZ_RGB, head_dim 16) is one of the cases,
    on sheet-like scenes whose windows hold 1 .. 58 tokens: one key per lane, one step of the gradient sweep.  Windows
    above 64 tokens (the fork's 7^3 windows on its coarse levels), bf16 and per-row checks of the table gradients are
    test_hip_swin3d_windows.py's."""
    from ptv3_hip import autograd as A
    coords = _surface(1500, 40, heads + hd + ws)
    q, k, v, tabs, offs, w_sizes, w2n, n2n, cr = _case(coords, heads, hd, ws, quant, crse, seed=3, table_std=0.3)
    assert w_sizes.min() < 16 < w_sizes.max() <= 64
    rng = np.random.default_rng(1)
    dout = rng.normal(size=q.shape).astype(np.float32)
    ref_in = [torch.from_numpy(a).double().requires_grad_(True) for a in (q, k, v, *tabs)]
    ref = _crse_attention_torch(*ref_in, offs, w_sizes, w2n, n2n, cr)
    ref.backward(torch.from_numpy(dout).double())
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    dev_in = [t(a).requires_grad_(True) for a in (q, k, v, *tabs)]
    w_start = t(np.concatenate([w2n, [len(q)]]).astype(np.int32))
    out = A.swin_attention(*dev_in, offs, t(n2n.astype(np.int64)), w_start, t(cr), int(w_sizes.max()))
    assert _rel(out.detach().cpu().numpy(), ref.detach().numpy()) <= 1e-4
    out.backward(t(dout))
    for name, a, b in zip(("dq", "dk", "dv", "dq_table", "dk_table", "dv_table"), dev_in, ref_in):
        assert _rel(a.grad.cpu().numpy(), b.grad.numpy()) <= 1e-4, (name, _rel(a.grad.cpu().numpy(), b.grad.numpy()))


def test_swin3d_train_step_gradients_by_directional_derivative(dev):
    """A whole "Swin3D-v1m1" training step under `DefaultSegmentor` (CrossEntropy): every parameter receives a finite
    gradient, and the gradient agrees with central finite differences of the loss along random directions (fp32,
    DropPath off, batch-statistic BatchNorm; geometry - voxels, windows, neighbours - does not depend on the
    parameters).  There is no second implementation of this model's backward to compare with (the reference's lives in
    MinkowskiEngine / microsoft/Swin3D): the finite differences check it against its own forward, which
    test_swin3d_unet_forward_matches_the_restated_model ties to the oracle."""
    from ptv3_hip import configs
    from pointcept.models import build_model
    cfg = dict(type="DefaultSegmentor", backbone=dict(configs.TINY_SWIN3D_CFG, drop_path_rate=0.0),
               criteria=[dict(type="CrossEntropyLoss", loss_weight=1.0, ignore_index=-1)])
    model = build_model(cfg)
    _randomise(model, 5)
    model = model.to(dev).train()
    batch = _to_dev(_swin_batch([1800, 1100], seed=8), dev)
    batch["segment"] = torch.from_numpy(np.random.default_rng(0).integers(0, 13, batch["coord"].shape[0])).to(dev)
    params = [p for p in model.parameters() if p.requires_grad]

    from pointcept.models.utils.hip_layers import DropPath
    for m in model.modules():      # the same function at every evaluation: running statistics frozen, no DropPath draw
        if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):     # (Upsample's attention block hard-codes
            m.momentum = 0.0                                         # drop_path 0.1, swin3d_layers.py:352)
        if isinstance(m, DropPath):
            m.drop_prob = 0.0

    def loss_of():
        return model(dict(batch))["loss"]

    loss = loss_of()
    loss.backward()
    grads = [p.grad.clone() for p in params]
    assert all(g is not None and torch.isfinite(g).all() for g in grads)
    named = dict(model.named_parameters())
    for key in ("backbone.stem_layer.conv_layers.0.kernel", "backbone.layers.0.blocks.0.attn.query_xyz_table",
                "backbone.layers.1.blocks.1.attn.value_norm_table", "backbone.layers.0.downsample.linear.weight",
                "backbone.upsamples.0.linear2.1.weight", "backbone.classifier.3.weight"):
        assert named[key].grad.abs().max().item() > 0, key
    # finite differences along random directions in the parameters downstream of the last max-pool (deepest stage, both
    # upsampling steps with their attention blocks, classifier).  Upstream of the two 16-neighbour max-pools the loss has
    # a kink wherever an arg-max changes hands and central differences stop converging (the same script per parameter:
    # upstream values wander with the step size, downstream ones sit within 5 % of the analytic value); the upstream
    # layers are checked piecewise instead - test_swin3d_stem_and_downsample_training_paths_vs_torch_autograd,
    # test_crse_attention_backward_vs_torch_autograd and the PTv3 path's Function tests.
    late = [(n_, p) for n_, p in model.named_parameters()
            if n_.startswith(("backbone.layers.2.", "backbone.upsamples.", "backbone.classifier."))]
    assert len(late) > 60
    gen = torch.Generator().manual_seed(1)
    for trial in range(3):
        dirs = [torch.randn(p.shape, generator=gen).to(dev) * p.detach().abs().mean().clamp_min(1e-3) for _, p in late]
        analytic = sum((p.grad * d).sum().item() for (_, p), d in zip(late, dirs))
        eps = 3e-3
        with torch.no_grad():
            for (_, p), d in zip(late, dirs):
                p.add_(d, alpha=eps)
            up = loss_of().item()
            for (_, p), d in zip(late, dirs):
                p.add_(d, alpha=-2 * eps)
            down = loss_of().item()
            for (_, p), d in zip(late, dirs):
                p.add_(d, alpha=eps)
        numeric = (up - down) / (2 * eps)
        assert abs(numeric - analytic) <= 0.05 * max(abs(numeric), abs(analytic)) + 1e-3, (trial, numeric, analytic)


def test_offset_keypoint_swin3d_trains(dev):
    """The fork's Swin3D offset model (quant 50, XYZ_RGB) over a few FusedAdamW steps: the loss goes down."""
    from pointcept.models import build_model
    from ptv3_hip.optim import FusedAdamW
    cfg = dict(type="OffsetKeypointSwin3D", num_keypoints=6, hidden_dim=32,
               backbone_conf=dict(type="Swin3D-v1m1", in_channels=4, num_classes=32, base_grid_size=0.02, quant_size=50,
                                  num_layers=3, depths=[2, 2, 2], channels=[32, 32, 64], num_heads=[2, 2, 4],
                                  window_sizes=[5, 7, 7], up_k=3, drop_path_rate=0.1, stem_transformer=True,
                                  down_stride=2, upsample="linear", knn_down=True, cRSE="XYZ_RGB", fp16_mode=1))
    torch.manual_seed(3)
    model = build_model(cfg).to(dev).train()
    batch = _swin_batch([1500, 1200], seed=2, sig_dim=4, feat_dim=4, dup=0.0)
    batch["feat"] = np.clip(batch.pop("coord_feat"), -1, 1)
    data = _to_dev(batch, dev)
    rng = np.random.default_rng(0)
    n = data["coord"].shape[0]
    data["target"] = torch.from_numpy(np.concatenate([rng.normal(size=(n, 6, 3)) * 0.3, (rng.random((n, 6, 1)) > 0.5)],
                                                     -1).astype(np.float32)).to(dev)
    opt = FusedAdamW(model.parameters(), lr=2e-3, weight_decay=0.01)
    losses = []
    for _ in range(8):
        opt.zero_grad()
        out = model(dict(data))
        # the curves the reference's InformationWriter logs for this class (offset_keypoint_swin3d.py:92-124)
        assert set(out) == {"loss", "train/cls_loss", "train/reg_loss", "train/offset_l1_err", "train/mean_dist"} | \
            {f"train/kp{i}_dist" for i in range(6)}
        assert all(v.dim() == 0 and not v.requires_grad for k, v in out.items() if k != "loss")
        assert abs(out["train/mean_dist"].item() - sum(out[f"train/kp{i}_dist"].item() for i in range(6)) / 6) < 1e-5
        out["loss"].backward()
        opt.step()
        losses.append(out["loss"].item())
    assert all(np.isfinite(losses)) and losses[-1] < 0.9 * losses[0], losses


def test_swin3d_stem_and_downsample_training_paths_vs_torch_autograd(dev):
    """The two Swin3D-only layers with a taped training path of their own, each against torch autograd (float64, CPU)
    over a restatement on the same geometry: the stem (MinkowskiConvolution kernel (27, cin, cout) re-indexed to this
    package's tap order as a differentiable view -> batch-statistic BatchNorm -> ReLU) and GridKNNDownsample's feature
    half (LayerNorm -> Linear -> max over the 16 gathered neighbours, where a source voxel feeds several outputs)."""
    import torch.nn.functional as F
    from oracle.ptv3 import subm_conv3d
    from pointcept.models.swin3d.swin3d_v1m1_base import _ConvBNRelu, GridKNNDownsample, _Level
    rng = np.random.default_rng(4)
    coords = _surface(1500, 36, 21)
    n = len(coords)
    x = rng.normal(size=(n, 9)).astype(np.float32)
    dy = rng.normal(size=(n, 16)).astype(np.float32)
    torch.manual_seed(0)
    stem = _ConvBNRelu(9, 16)
    with torch.no_grad():
        stem.conv_layers[1].bn.weight.uniform_(0.5, 1.5)
        stem.conv_layers[1].bn.bias.normal_(0, 0.2)
    kern = stem.conv_layers[0].kernel.detach().double().requires_grad_(True)
    g = stem.conv_layers[1].bn.weight.detach().double().requires_grad_(True)
    b = stem.conv_layers[1].bn.bias.detach().double().requires_grad_(True)
    w = torch.stack([torch.stack([torch.stack([kern[a + 3 * bb + 9 * c].t() for c in range(3)], 1) for bb in range(3)], 1)
                     for a in range(3)], 1)                                  # (cout, 3, 3, 3, cin), x fastest in `kernel`
    y = subm_conv3d(torch.from_numpy(x).double(), torch.from_numpy(coords.astype(np.int64)), w)
    ref = F.relu(F.batch_norm(y, None, None, g, b, True, 0.0, 1e-5))
    ref.backward(torch.from_numpy(dy).double())
    stem = stem.to(dev).train()
    level = _Level(torch.from_numpy(coords).to(dev), 1, torch.from_numpy(x).to(dev), None, None)
    out = stem(level).feat
    assert _rel(out.detach().cpu().numpy(), ref.detach().numpy()) <= 1e-4
    out.backward(torch.from_numpy(dy).to(dev))
    for name, got, want in (("kernel", stem.conv_layers[0].kernel.grad, kern.grad),
                            ("bn.weight", stem.conv_layers[1].bn.weight.grad, g.grad),
                            ("bn.bias", stem.conv_layers[1].bn.bias.grad, b.grad)):
        assert _rel(got.cpu().numpy(), want.numpy()) <= 2e-4, (name, _rel(got.cpu().numpy(), want.numpy()))

    # ---- GridKNNDownsample: features through LayerNorm, Linear and the max over 16 gathered rows
    down = GridKNNDownsample(16, 32, kernel_size=3, stride=3)
    with torch.no_grad():
        down.norm.weight.uniform_(0.5, 1.5)
        down.norm.bias.normal_(0, 0.2)
    feat = rng.normal(size=(n, 16)).astype(np.float32)
    cfeat = np.concatenate([np.zeros((n, 1)), coords[:, 1:] + rng.random((n, 3)), rng.uniform(-1, 1, (n, 6))], 1)
    cfeat = cfeat.astype(np.float32)
    offset = torch.tensor([n], dtype=torch.int32, device=dev)
    down = down.to(dev).train()
    fin = torch.from_numpy(feat).to(dev).requires_grad_(True)
    lv = _Level(torch.from_numpy(coords).to(dev), 1, fin, torch.from_numpy(cfeat).to(dev), offset)
    # the neighbour indices the module will use (same call as inside it), for the reference
    import pointops
    coarse = down(lv)
    idx, _ = pointops.knn_query(16, lv.xyz, lv.offset, coarse.cfeat[:, 1:4].contiguous(), coarse.offset, cell=1.0)
    idx = torch.where(idx < 0, idx[:, :1], idx).long().cpu()
    dyc = rng.normal(size=tuple(coarse.feat.shape)).astype(np.float32)
    coarse.feat.backward(torch.from_numpy(dyc).to(dev))
    fr = torch.from_numpy(feat).double().requires_grad_(True)
    wn, bn_, wl = (p.detach().cpu().double().requires_grad_(True) for p in (down.norm.weight, down.norm.bias,
                                                                          down.linear.weight))
    yr = F.layer_norm(fr, (16,), wn, bn_, 1e-5) @ wl.t()
    ref2 = yr[idx].max(dim=1).values
    assert _rel(coarse.feat.detach().cpu().numpy(), ref2.detach().numpy()) <= 1e-4
    ref2.backward(torch.from_numpy(dyc).double())
    for name, got, want in (("feat", fin.grad, fr.grad), ("norm.weight", down.norm.weight.grad, wn.grad),
                            ("norm.bias", down.norm.bias.grad, bn_.grad), ("linear.weight", down.linear.weight.grad, wl.grad)):
        assert _rel(got.cpu().numpy(), want.numpy()) <= 2e-4, (name, _rel(got.cpu().numpy(), want.numpy()))
