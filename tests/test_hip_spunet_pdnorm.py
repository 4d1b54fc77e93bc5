"""SpUNet-v1m3 on the GPU: the one-launch modulation kernels (csrc/pdnorm.hip) against tests/pdnorm_ref.py in float64, the
model under PPT-v1m2 against the reference's own outputs (tests/golden/spunet_pdnorm_*.npz), the fused eval forward against
the composition, the launch accounting of the modulation path, one training step, and the configs end to end.

Kernel tolerance (the rule of test_hip_ppt.py): the kernel's largest error against the float64
yardstick may be at most four times that of the same statement order evaluated by torch in float32 on the device, with a
floor of 8 float32 ulps of the largest entry.  Model tolerances are those of test_hip_keypoint_spunet.py."""
import numpy as np
import pytest
import torch

import pdnorm_ref as R
from make_golden_spunet_pdnorm import (load_golden, tiny_kw, tiny_backbone, pdnorm_state_dict, batch_of, CONDITIONS, TAPS,
                                       TAP_STRIDE, PD_TAP, EVAL_CONDITIONS, TRAIN_CONDITION, HEAD_PREFIX)
from test_hip_keypoint_oacnns import FP32_TOL

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -23
EPS = 1e-3
LAYER_SETS = {"one": (4,), "odd": (4, 20, 96), "wide": (16, 32, 32, 64, 256, 260), "tiny": None}   # None: the tiny model's 33
LAYERS = (1, 2, 1, 1, 1, 1, 2, 1)


def _widths(name):
    if LAYER_SETS[name] is None:
        from pointcept.models import build_model
        LAYER_SETS[name] = tuple(m.num_features for m in build_model(tiny_backbone("affine")).pdnorms())
        assert len(LAYER_SETS[name]) == 33
    return LAYER_SETS[name]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X box"
    return torch.device("cuda:0")


def _rule(name, got, ref32, ref64):
    ref64 = ref64.detach().cpu().double()
    err_k = (got.detach().cpu().double() - ref64).abs().max().item()
    err_t = (ref32.detach().cpu().double() - ref64).abs().max().item()
    top = ref64.abs().max().item()
    bound = max(4.0 * err_t, 8.0 * ULP * top)
    print(f"{name}: kernel {err_k:.3e} torch-fp32 {err_t:.3e} max|ref| {top:.3e} bound {bound:.3e}")
    assert err_k <= bound, (name, err_k, err_t, top)


def _table(layers):
    from ptv3_hip import ops
    return ops.pdnorm_table([(ly["W"], ly["b"], ly["gamma"], ly["beta"], ly["mean"], ly["var"]) for ly in layers])


def _cat(parts):
    return torch.cat([p.reshape(-1) for p in parts])


# ------------------------------------------------------------------------------------------------
# the kernels
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cc", [1, 24, 100, 256])
@pytest.mark.parametrize("widths", list(LAYER_SETS))
def test_modulation_kernels_against_float64(dev, widths, cc):
    """forward (train and fold mode) and backward, affine on and off, contexts of magnitude 0.1 and 20 (the SiLU tails),
    running_var down to 1e-6; two runs bitwise equal"""
    from ptv3_hip import ops
    ws = _widths(widths)
    assert all(ops.pdnorm_capable(c, cc) for c in ws)
    for affine in (True, False):
        for magnitude in (0.1, 20.0):
            seed = 100 * cc + int(magnitude) + int(affine)
            l64, c64 = R.make_layers(ws, cc, affine, seed, magnitude=magnitude)
            l32, c32 = R.make_layers(ws, cc, affine, seed, dtype=torch.float32, device=dev, magnitude=magnitude)
            tab = _table(l32)
            tag = f"{widths} Cc={cc} affine={affine} |ctx|~{magnitude}"
            for fold in (False, True):
                o0, o1, op = ops.pdnorm_fwd(tab, c32.view(-1), fold=fold, eps=EPS)
                again = ops.pdnorm_fwd(tab, c32.view(-1), fold=fold, eps=EPS)
                assert all(torch.equal(a, b) for a, b in zip((o0, o1, op), again))
                want = R.forward(c64, l64, fold=fold, eps=EPS)
                with torch.no_grad():
                    t32 = R.forward(c32, l32, fold=fold, eps=EPS)
                for j, (got, nm) in enumerate(((o0, "out0"), (o1, "out1"), (op, "1+scale"))):
                    _rule(f"{tag} fold={fold} {nm}", got, _cat([t[j] for t in t32]), _cat([w[j] for w in want]))
            # backward
            g = torch.Generator().manual_seed(seed + 7)
            d0 = [torch.randn(c, generator=g, dtype=torch.float64).float() for c in ws]
            d1 = [torch.randn(c, generator=g, dtype=torch.float64).float() for c in ws]
            want, want_ctx = R.backward(c64, l64, [d.double() for d in d0], [d.double() for d in d1])
            leaves = [c32] + [t for ly in l32 for t in (ly["W"], ly["b"], ly["gamma"], ly["beta"]) if t is not None]
            for t in leaves:
                t.requires_grad_(True)
            loss = sum((ge * a.to(dev)).sum() + (be * b.to(dev)).sum()
                       for (ge, be, _), a, b in zip(R.forward(c32, l32), d0, d1))
            loss.backward()
            _, _, op = ops.pdnorm_fwd(tab, c32.detach().view(-1))
            p0, p1 = _cat(d0).to(dev), _cat(d1).to(dev)
            got = ops.pdnorm_bwd(tab, c32.detach().view(-1), p0, p1, op)
            again = ops.pdnorm_bwd(tab, c32.detach().view(-1), p0, p1, op)
            assert all((a is None and b is None) or torch.equal(a, b) for a, b in zip(got, again))
            dW, db, dgamma, dbeta, dctx = got
            _rule(f"{tag} dW", dW.view(-1), _cat([ly["W"].grad for ly in l32]), _cat([w[0] for w in want]))
            _rule(f"{tag} db", db, _cat([ly["b"].grad for ly in l32]), _cat([w[1] for w in want]))
            _rule(f"{tag} dcontext", dctx, c32.grad.view(-1), want_ctx.view(-1))
            if affine:
                _rule(f"{tag} dgamma", dgamma, _cat([ly["gamma"].grad for ly in l32]), _cat([w[2] for w in want]))
                _rule(f"{tag} dbeta", dbeta, _cat([ly["beta"].grad for ly in l32]), _cat([w[3] for w in want]))
            else:
                assert dgamma is None and dbeta is None


def test_pointer_table_survives_in_place_updates(dev):
    """the table holds addresses: an in-place optimizer step needs no new table and gives fresh values; a parameter
    replaced by a new tensor changes the key"""
    from ptv3_hip import ops
    l32, c32 = R.make_layers((4, 20, 96), 24, True, 3, dtype=torch.float32, device=dev)
    params = [torch.nn.Parameter(ly[k]) for ly in l32 for k in ("W", "b", "gamma", "beta")]
    for ly, i in zip(l32, range(0, len(params), 4)):
        ly["W"], ly["b"], ly["gamma"], ly["beta"] = params[i:i + 4]
    as_tuples = lambda: [(ly["W"], ly["b"], ly["gamma"], ly["beta"], ly["mean"], ly["var"]) for ly in l32]
    tab = ops.pdnorm_table(as_tuples())
    before = ops.pdnorm_fwd(tab, c32.view(-1))[0].clone()
    for p in params:
        p.grad = torch.ones_like(p)
    torch.optim.SGD(params, lr=0.05).step()
    assert tab.key == ops.pdnorm_table_key(as_tuples())
    after = ops.pdnorm_fwd(tab, c32.view(-1))[0]
    assert not torch.equal(before, after)
    with torch.no_grad():
        want = _cat([t[0] for t in R.forward(c32.double(), [{k: None if v is None else v.detach().double()
                                                               for k, v in ly.items()} for ly in l32])])
    assert (after.double() - want).abs().max().item() <= 8 * ULP * want.abs().max().item()
    l32[1]["W"] = torch.nn.Parameter(l32[1]["W"].detach().clone())
    assert tab.key != ops.pdnorm_table_key(as_tuples())


# ------------------------------------------------------------------------------------------------
# the model against the reference fixture
# ------------------------------------------------------------------------------------------------
_GOLDEN = {}


def _golden(golden_dir, variant):
    if variant not in _GOLDEN:
        _GOLDEN[variant] = load_golden(golden_dir, variant)
    return _GOLDEN[variant]


def _tiny(golden_dir, dev, variant="affine", modulation=None):
    from pointcept.models import build_model
    g = _golden(golden_dir, variant)
    model = build_model(dict(type="PPT-v1m2", **tiny_kw(variant)))
    pdnorm_state_dict(model)
    model.backbone.set_modulation(modulation)
    data = {k[3:]: torch.from_numpy(v).to(dev) for k, v in _golden(golden_dir, "affine").items() if k.startswith("in_")}
    return g, model.to(dev), data


def _tapped_eval(model, data, cond, with_segment=True):
    taps = []
    inner = model.backbone.forward
    model.backbone.forward = lambda d: inner(d, taps=taps)
    try:
        with torch.no_grad():
            out = model.eval()(batch_of(data, cond, with_segment=with_segment))
    finally:
        del model.backbone.forward
    assert len(taps) == len(TAPS)
    return out, dict(zip(TAPS, taps))


def _stored(feat, n_in):
    return feat[::TAP_STRIDE] if feat.shape[0] == n_in else feat


def _count(monkeypatch, name):
    from ptv3_hip import ops
    calls, inner = [], getattr(ops, name)

    def counting(*a, **k):
        calls.append((a, k))
        return inner(*a, **k)
    monkeypatch.setattr(ops, name, counting)
    return calls


@pytest.mark.parametrize("modulation", [True, False])
def test_eval_vs_reference_golden(dev, golden_dir, monkeypatch, modulation):
    """Coarse site lists exactly; the nine taps, seg_logits and the loss under "B" and "C" within FP32_TOL of each
    tensor's scale; with the kernel forced on, every block's conv2 and the 4 decoder fronts run ptv3_res_conv."""
    g, model, data = _tiny(golden_dir, dev, modulation=modulation)
    model.backbone.set_res_conv(True)
    n_in = data["feat"].shape[0]
    for cond in EVAL_CONDITIONS:
        calls = _count(monkeypatch, "res_conv")
        out, taps = _tapped_eval(model, data, cond)
        monkeypatch.undo()
        assert len(calls) == sum(LAYERS) + 4
        for i in range(4):
            assert np.array_equal(taps[f"enc.{i}"].indices.cpu().numpy(), g[f"sites{i + 1}"]), i
        for name in TAPS:
            ref = g[f"tap_{cond}_{name}"]
            err = np.abs(_stored(taps[name].features, n_in).cpu().numpy() - ref).max()
            print(f"{cond} tap {name}: error {err:.3e}, scale {np.abs(ref).max():.3e}")
            assert err < FP32_TOL * np.abs(ref).max(), (cond, name, err)
        ref = g[f"eval_seg_logits_{cond}"]
        assert out["seg_logits"].shape == ref.shape
        assert np.abs(out["seg_logits"].cpu().numpy() - ref).max() < FP32_TOL * max(1.0, np.abs(ref).max())
        assert abs(out["loss"].item() - float(g[f"eval_loss_{cond}"])) < FP32_TOL


@pytest.mark.parametrize("variant", ["noaffine", "plain"])
def test_variants_eval_vs_reference_golden(dev, golden_dir, variant):
    for modulation in ((True, False) if variant == "noaffine" else (None,)):
        g, model, data = _tiny(golden_dir, dev, variant, modulation)
        with torch.no_grad():
            out = model.eval()(batch_of(data, TRAIN_CONDITION))
        ref = g[f"eval_seg_logits_{TRAIN_CONDITION}"]
        assert np.abs(out["seg_logits"].cpu().numpy() - ref).max() < FP32_TOL * max(1.0, np.abs(ref).max())
        assert abs(out["loss"].item() - float(g[f"eval_loss_{TRAIN_CONDITION}"])) < FP32_TOL


def test_one_pdbatchnorm_vs_reference_golden(dev, golden_dir):
    """the stored input -> output pair of one PDBatchNorm under "B", in eval and in training mode, called with the
    reference's signature (feat, condition, context)"""
    g, model, data = _tiny(golden_dir, dev)
    pd = dict(model.named_modules())[PD_TAP]
    idx = torch.tensor([CONDITIONS.index(TRAIN_CONDITION)], device=dev)
    for mode in ("eval", "train"):
        model.train(mode == "train")
        x = torch.from_numpy(g[f"{mode}_pd_in"]).to(dev)
        with torch.no_grad():
            y = pd(x, TRAIN_CONDITION, model.embedding_table(idx))
        ref = g[f"{mode}_pd_out"]
        err = np.abs(y.cpu().numpy() - ref).max()
        print(f"{mode}: error {err:.3e}, scale {np.abs(ref).max():.3e}")
        assert err < FP32_TOL * np.abs(ref).max(), (mode, err)


def _compare(g, cond, name_a, a_taps, b_taps, n_in):
    """every row of every tap: |a - b| at most 4x b's own distance from the reference's fp32 run on the stored rows"""
    for name in TAPS:
        a, b, ref = a_taps[name].features, b_taps[name].features, g[f"tap_{cond}_{name}"]
        err = (a - b).abs().max().item()
        base = np.abs(_stored(b, n_in).cpu().numpy() - ref).max()
        print(f"tap {name}: {name_a} {err:.3e}, composed - reference {base:.3e}")
        assert err <= max(4 * base, 2.0 ** -23 * np.abs(ref).max()), (name, err, base)


@pytest.mark.parametrize("modulation", [True, False])
def test_fused_eval_and_kernel_wiring_vs_composition(dev, golden_dir, monkeypatch, modulation):
    """The fused eval forward (default wiring), set_res_conv(True) and set_res_conv(False) against set_fused(False); the
    yardstick is the composition's own fp32 distance from the fixture."""
    g, model, data = _tiny(golden_dir, dev, modulation=modulation)
    cond, n_in = TRAIN_CONDITION, data["feat"].shape[0]
    fused, taps = _tapped_eval(model, data, cond)
    calls = _count(monkeypatch, "res_conv")
    model.backbone.set_res_conv(True)
    on, on_taps = _tapped_eval(model, data, cond)
    assert len(calls) == sum(LAYERS) + 4
    del calls[:]
    model.backbone.set_res_conv(False)
    off, off_taps = _tapped_eval(model, data, cond)
    assert not calls
    model.backbone.set_fused(False)
    plain, ref_taps = _tapped_eval(model, data, cond)
    _compare(g, cond, "fused - composed", taps, ref_taps, n_in)
    _compare(g, cond, "kernel on - composed", on_taps, ref_taps, n_in)
    _compare(g, cond, "kernel off - composed", off_taps, ref_taps, n_in)
    for out in (fused, on, off):
        assert (out["seg_logits"] - plain["seg_logits"]).abs().max().item() < FP32_TOL * max(
            1.0, plain["seg_logits"].abs().max().item())
        assert abs(out["loss"].item() - plain["loss"].item()) < FP32_TOL


def test_modulation_launch_accounting(dev, golden_dir, monkeypatch):
    """With the one-launch path on: a training forward + backward calls the modulation forward once and its backward
    once and no GEMM with one row; a second eval forward launches neither modulation nor fold; an optimizer step and a
    change of condition cost exactly one fold each."""
    g, model, data = _tiny(golden_dir, dev, modulation=True)
    fwd, bwd, gemm = _count(monkeypatch, "pdnorm_fwd"), _count(monkeypatch, "pdnorm_bwd"), _count(monkeypatch, "gemm")
    opt = torch.optim.SGD(model.parameters(), lr=1e-3)
    model.train()
    out = model(batch_of(data, TRAIN_CONDITION))
    out["loss"].backward()
    assert len(fwd) == 1 and not fwd[0][1].get("fold", False) and len(bwd) == 1
    assert gemm and not [1 for a, k in gemm if a[0].shape[0] == 1]
    del fwd[:], bwd[:]
    model.eval()
    with torch.no_grad():
        model(batch_of(data, TRAIN_CONDITION, with_segment=False))
        assert len(fwd) == 1 and fwd[0][1].get("fold") is True
        model(batch_of(data, TRAIN_CONDITION, with_segment=False))
        assert len(fwd) == 1 and not bwd
        opt.step()
        model(batch_of(data, TRAIN_CONDITION, with_segment=False))
        assert len(fwd) == 2
        model(batch_of(data, "C", with_segment=False))
        assert len(fwd) == 3
        model(batch_of(data, TRAIN_CONDITION, with_segment=False))
        model(batch_of(data, "C", with_segment=False))
        assert len(fwd) == 3 and not bwd
    assert not [1 for a, k in gemm if a[0].shape[0] == 1]


def test_model_table_is_rebuilt_only_for_a_replaced_parameter(dev, golden_dir):
    g, model, data = _tiny(golden_dir, dev, modulation=True)
    bb = model.backbone
    opt = torch.optim.SGD(model.parameters(), lr=1e-3)
    model.train()
    model(batch_of(data, TRAIN_CONDITION))["loss"].backward()
    (tab,) = bb._tables.values()
    opt.step()
    model.zero_grad()
    model(batch_of(data, TRAIN_CONDITION))["loss"].backward()
    assert list(bb._tables.values()) == [tab]
    lin = bb.pdnorms()[3].modulation[1]
    lin.weight = torch.nn.Parameter(lin.weight.detach().clone())
    model.zero_grad()
    model(batch_of(data, TRAIN_CONDITION))["loss"].backward()
    (new,) = bb._tables.values()
    assert new is not tab and lin.weight.grad is not None and lin.weight.grad.abs().max().item() > 0


@pytest.mark.parametrize("modulation", [True, False])
def test_eval_reads_the_device_five_times(dev, golden_dir, monkeypatch, modulation):
    """One read at entry (spatial shape and offsets) and one per stage; counted as in test_hip_keypoint_spunet.py."""
    g, model, data = _tiny(golden_dir, dev, modulation=modulation)
    model.eval()
    with torch.no_grad():
        model(batch_of(data, TRAIN_CONDITION, with_segment=False))            # parameter caches filled
    reads = []
    for name in ("tolist", "item", "cpu", "numpy"):
        inner = getattr(torch.Tensor, name)

        def counting(self, *a, _inner=inner, _name=name, **k):
            if self.is_cuda:
                reads.append(_name)
            return _inner(self, *a, **k)
        monkeypatch.setattr(torch.Tensor, name, counting)
    with torch.no_grad():
        out = model(batch_of(data, TRAIN_CONDITION, with_segment=False))
    monkeypatch.undo()
    assert reads == ["tolist"] * 5, reads
    ref = g[f"eval_seg_logits_{TRAIN_CONDITION}"]
    assert np.abs(out["seg_logits"].cpu().numpy() - ref).max() < FP32_TOL * max(1.0, np.abs(ref).max())


def _check_train_step(g, model, data, full):
    model.train()
    out = model(batch_of(data, TRAIN_CONDITION))
    out["loss"].backward()
    assert abs(out["loss"].item() - float(g["train_loss"])) < 1e-4, (out["loss"].item(), float(g["train_loss"]))
    grads = {k[5:]: g[k].astype(np.float32) * g["gmax_" + k[5:]] for k in g if k.startswith("grad_") and k != "grad_parts"}
    gmax = float(g["gmax_all"])
    params = dict(model.named_parameters())
    if full:
        nograd = sorted(n for n, p in params.items() if p.grad is None)
        assert nograd == sorted(str(n) for n in g["nograd"])
        assert set(grads) == set(params) - set(nograd)
        assert any(n.endswith("modulation.1.weight") for n in grads) and "embedding_table.weight" in grads
    worst = ("", 0.0)
    for n, ref in grads.items():
        assert params[n].grad is not None, n
        err = np.abs(params[n].grad.float().cpu().numpy() - ref).max() / max(np.abs(ref).max(), 1e-3 * gmax)
        worst = max(worst, (n, err), key=lambda q: q[1])
        assert err < (2e-3 if n.startswith(HEAD_PREFIX) else 1e-2), (n, err)
    print("worst gradient error", worst)
    return out


@pytest.mark.parametrize("modulation", [True, False])
def test_train_step_vs_reference_golden(dev, golden_dir, modulation):
    """Loss, every parameter gradient (every modulation Linear and embedding_table.weight included), the names without a
    gradient and every running buffer of one training step under "B", with check_step's tolerances."""
    g, model, data = _tiny(golden_dir, dev, modulation=modulation)
    _check_train_step(g, model, data, full=True)
    active = f".bns.{CONDITIONS.index(TRAIN_CONDITION)}."
    for n, b in model.named_buffers():
        ref = torch.from_numpy(g["buf_" + n])
        if n.endswith("num_batches_tracked"):
            assert b.item() == ref.item() == (1 if active in n else 0), n
        else:
            assert (b.cpu() - ref).abs().max().item() / max(ref.abs().max().item(), 1e-6) < 1e-4, n


@pytest.mark.parametrize("variant", ["noaffine", "plain"])
def test_variants_train_step_vs_reference_golden(dev, golden_dir, variant):
    for modulation in ((True, False) if variant == "noaffine" else (None,)):
        g, model, data = _tiny(golden_dir, dev, variant, modulation)
        _check_train_step(g, model, data, full=False)
        if variant == "noaffine":
            assert "embedding_table.weight" in [k[5:] for k in g if k.startswith("grad_")]


# ------------------------------------------------------------------------------------------------
# end to end
# ------------------------------------------------------------------------------------------------
def test_scannet_config_eval_and_train_step(dev):
    """PPT_SPUNET_SCANNET_CFG (59 PDBatchNorms) with seeded class embeddings on two scenes of 3000 sites"""
    import ptv3_scenes as S
    from pointcept.models import build_model
    from ptv3_hip.configs import PPT_SPUNET_SCANNET_CFG
    torch.manual_seed(7)
    model = build_model(PPT_SPUNET_SCANNET_CFG)
    model.set_class_embedding(torch.randn(tuple(model.class_embedding.shape), generator=torch.Generator().manual_seed(1)))
    model = model.to(dev)
    data = {k: v.to(dev) for k, v in S.make_batch([3000, 3000], in_channels=6, extent=64, seed=3).items()}
    n = data["feat"].shape[0]
    data["segment"] = torch.randint(0, 20, (n,), device=dev)
    data["condition"] = ["ScanNet"]
    for modulation in (True, False):
        model.backbone.set_modulation(modulation)
        with torch.no_grad():
            logits = model.eval()(dict(data))["seg_logits"]
        assert tuple(logits.shape) == (n, 20) and torch.isfinite(logits).all()
    opt = torch.optim.AdamW(model.parameters(), lr=2e-3, weight_decay=0.05)
    out = model.train()(dict(data))
    out["loss"].backward()
    opt.step()
    assert torch.isfinite(out["loss"]).item()
    assert all(torch.isfinite(p).all() and (p.grad is None or torch.isfinite(p.grad).all()) for p in model.parameters())
    # 59 PDBatchNorms x (W, b, gamma, beta) of the active condition, 59 conv weights, embedding_table and proj_head
    assert sum(p.grad is not None for p in model.parameters()) == 4 * 59 + 59 + 3


def test_pointgroup_over_ppt_backbone_mode_runs(dev, golden_dir):
    """PG-v1m1 over PPT-v1m1(backbone_mode=True) over the tiny SpUNet-v1m3: builds and runs one eval forward"""
    from pointcept.models import build_model
    g, _, data = _tiny(golden_dir, dev)
    model = build_model(dict(
        type="PG-v1m1",
        backbone=dict(type="PPT-v1m1", backbone=tiny_backbone("affine"), backbone_out_channels=16, context_channels=24,
                      conditions=CONDITIONS, backbone_mode=True,
                      criteria=[dict(type="CrossEntropyLoss", loss_weight=1.0, ignore_index=-1)]),
        backbone_out_channels=16, semantic_num_classes=5, semantic_ignore_index=-1, segment_ignore_index=(-1, 0),
        instance_ignore_index=-1, cluster_thresh=1.5, cluster_closed_points=300, cluster_propose_points=100,
        cluster_min_points=50, voxel_size=0.02))
    pdnorm_state_dict(model.backbone)
    model = model.to(dev).eval()
    batch = batch_of(data, TRAIN_CONDITION, with_segment=False)
    batch["instance_centroid"] = batch["coord"].clone()
    with torch.no_grad():
        out = model(batch)
    n = data["feat"].shape[0]
    assert sorted(out.keys()) == ["pred_classes", "pred_masks", "pred_scores"]
    assert out["pred_masks"].shape[1] == n and out["pred_scores"].shape[0] == out["pred_masks"].shape[0]


def test_default_segmentor_fused_vs_composition(dev, golden_dir):
    """DefaultSegmentor (which unwraps the condition list to a string) over a non-adaptive, affine SpUNet-v1m3 with its
    `final` conv: fused eval against the composition"""
    from pointcept.models import build_model
    g, _, data = _tiny(golden_dir, dev)
    bb = dict(tiny_backbone("affine"), num_classes=13, norm_adaptive=False, norm_affine=True)
    model = build_model(dict(type="DefaultSegmentor", backbone=bb,
                             criteria=[dict(type="CrossEntropyLoss", loss_weight=1.0, ignore_index=-1)]))
    pdnorm_state_dict(model.backbone)
    model = model.to(dev).eval()
    with torch.no_grad():
        fused = model(batch_of(data, TRAIN_CONDITION, with_segment=False))["seg_logits"]
        model.backbone.set_fused(False)
        plain = model(batch_of(data, TRAIN_CONDITION, with_segment=False))["seg_logits"]
    assert not model.backbone._tables          # no modulation: a PDBatchNorm is exactly its active BatchNorm1d
    assert tuple(fused.shape) == (data["feat"].shape[0], 13) and torch.isfinite(fused).all()
    assert (fused - plain).abs().max().item() < FP32_TOL * max(1.0, plain.abs().max().item())


# ------------------------------------------------------------------------------------------------
# cache keys, alignment, the saved parameters
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("modulation", [True, False])
def test_shared_batchnorm_switches_condition_in_fused_eval(dev, golden_dir, modulation):
    """norm_decouple=False, norm_adaptive=True under PPT: the BatchNorm and embedding_table.weight are the same for every
    condition, only the context row differs, and the fold caches must tell the conditions apart.  Fused eval, switching
    condition back and forth, against set_fused(False)."""
    from pointcept.models import build_model
    g, _, data = _tiny(golden_dir, dev)
    kw = tiny_kw("affine")
    kw["backbone"] = dict(kw["backbone"], norm_decouple=False)
    model = build_model(dict(type="PPT-v1m2", **kw))
    pdnorm_state_dict(model)
    model = model.to(dev).eval()
    model.backbone.set_modulation(modulation)
    order = ("B", "C", "B", "A", "C")
    with torch.no_grad():
        fused = [model.backbone(_with_context(model, data, c)) for c in order]
        model.backbone.set_fused(False)
        plain = {c: model.backbone(_with_context(model, data, c)) for c in set(order)}
    assert (plain["B"] - plain["C"]).abs().max().item() > 1e-2 * plain["B"].abs().max().item()   # the conditions differ
    for c, out in zip(order, fused):
        err = (out - plain[c]).abs().max().item()
        assert err < FP32_TOL * max(1.0, plain[c].abs().max().item()), (c, err)


def _with_context(model, data, cond):
    batch = batch_of(data, cond, with_segment=False)
    idx = torch.tensor([CONDITIONS.index(cond)], device=data["feat"].device)
    batch["context"] = model.embedding_table(idx)
    batch["context_source"] = model.embedding_table.weight
    return batch


def test_fold_cache_without_a_source_follows_the_context_values(dev, golden_dir):
    """no context_source: the cache entry holds the context tensor it was computed from, so while it lives no later
    context can be handed its address; new values under the same condition are a miss and give new folds"""
    g, model, data = _tiny(golden_dir, dev, modulation=True)
    bb = model.backbone.eval()
    gen = torch.Generator().manual_seed(2)
    with torch.no_grad():
        for _ in range(4):
            ctx = torch.randn(1, 24, generator=gen).to(dev)
            got = bb.set_modulation(True).modulation_folds("B", ctx)
            assert bb._folds[("B", ctx.device)][2] is ctx
            want = ctx.clone()
            del ctx
            prompt = bb.set_modulation(False)._prompt(dict(condition="B", context=want))
            for m, (s, t) in zip(bb.pdnorms(), got):
                s0, t0 = m.folded(prompt)
                assert (s - s0).abs().max().item() <= 1e-5 * s0.abs().max().item()
                assert (t - t0).abs().max().item() <= 1e-5 * max(1.0, t0.abs().max().item())


def test_kernels_with_a_weight_off_the_16_byte_boundary(dev):
    """W as a contiguous view one float into its buffer, Cc % 4 == 0: the 4-byte loads of the forward and the gathered
    loads of the vector backward, against the aligned run of the same values (bitwise in forward: the lane-to-k mapping
    differs, so within the rule instead) and against float64"""
    from ptv3_hip import ops
    ws, cc = (4, 20, 96), 24
    l64, c64 = R.make_layers(ws, cc, True, 11, magnitude=1.0)
    l32, c32 = R.make_layers(ws, cc, True, 11, dtype=torch.float32, device=dev, magnitude=1.0)
    for ly in l32:
        buf = torch.empty(ly["W"].numel() + 1, device=dev)
        buf[1:] = ly["W"].reshape(-1)
        ly["W"] = buf[1:].view_as(ly["W"])
        assert ly["W"].is_contiguous() and ly["W"].data_ptr() % 16 == 4
    tab = _table(l32)
    for fold in (False, True):
        o0, o1, op = ops.pdnorm_fwd(tab, c32.view(-1), fold=fold, eps=EPS)
        want = R.forward(c64, l64, fold=fold, eps=EPS)
        t32 = R.forward(c32, l32, fold=fold, eps=EPS)
        for j, (got, nm) in enumerate(((o0, "out0"), (o1, "out1"), (op, "1+scale"))):
            _rule(f"unaligned W fold={fold} {nm}", got, _cat([t[j] for t in t32]), _cat([w[j] for w in want]))
    gen = torch.Generator().manual_seed(5)
    d0 = [torch.randn(c, generator=gen, dtype=torch.float64).float() for c in ws]
    d1 = [torch.randn(c, generator=gen, dtype=torch.float64).float() for c in ws]
    want, want_ctx = R.backward(c64, l64, [d.double() for d in d0], [d.double() for d in d1])
    leaves = [c32] + [ly["W"] for ly in l32]
    for t in leaves:
        t.requires_grad_(True)
    sum((ge * a.to(dev)).sum() + (be * b.to(dev)).sum() for (ge, be, _), a, b in zip(R.forward(c32, l32), d0, d1)).backward()
    _, _, op = ops.pdnorm_fwd(tab, c32.detach().view(-1))
    dW, db, dgamma, dbeta, dctx = ops.pdnorm_bwd(tab, c32.detach().view(-1), _cat(d0).to(dev), _cat(d1).to(dev), op)
    _rule("unaligned W dW", dW.view(-1), _cat([ly["W"].grad for ly in l32]), _cat([w[0] for w in want]))
    _rule("unaligned W dcontext", dctx, c32.grad.view(-1), want_ctx.view(-1))


def test_folded_pairs_start_on_16_bytes_behind_an_odd_width(dev):
    """a width that is no multiple of 4 (channels[-1] = 18) shifts every later slice of the packed fold buffer off the
    16-byte boundary ptv3_res_conv reads at: the model then hands out pairs with storage of their own.  No conv runs."""
    from pointcept.models import build_model
    kw = dict(tiny_backbone("affine"), channels=(16, 32, 32, 64, 64, 32, 16, 18))
    bb = build_model(kw)
    pdnorm_state_dict(bb)
    bb = bb.to(dev).eval()
    assert any(m.num_features == 18 for m in bb.pdnorms())
    ctx = torch.randn(1, 24, generator=torch.Generator().manual_seed(4)).to(dev)
    with torch.no_grad():
        pairs = bb.modulation_folds("B", ctx)
        bb.set_modulation(False)
        ref = [m.folded(bb._prompt(dict(condition="B", context=ctx))) for m in bb.pdnorms()]
    for m, (s, t), (s0, t0) in zip(bb.pdnorms(), pairs, ref):
        assert s.data_ptr() % 16 == 0 and t.data_ptr() % 16 == 0 and s.shape == (m.num_features,)
        assert (s - s0).abs().max().item() <= 1e-5 * s0.abs().max().item()
        assert (t - t0).abs().max().item() <= 1e-5 * max(1.0, t0.abs().max().item())


def test_parameter_changed_between_forward_and_backward_is_an_error(dev, golden_dir):
    """the backward reads the parameters through the address table; they are saved on the tape, so torch's version check
    refuses an in-place change in between, as it does for its own Linear"""
    g, model, data = _tiny(golden_dir, dev, modulation=True)
    bb = model.backbone.train()
    ctx = torch.randn(1, 24, device=dev, requires_grad=True)
    pairs = bb.modulation_pairs("B", ctx)
    with torch.no_grad():
        bb.pdnorms()[2].modulation[1].weight.mul_(1.5)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        sum(a.sum() + b.sum() for a, b in pairs).backward()
