"""ClsEvaluator / SemSegEvaluator / InsSegEvaluator on CPU tensors against tests/golden/seg_evaluators.npz, which holds what
the reference's hooks reported on the same batches (tests/golden/make_golden_seg_evaluators.py).  Counts and association
tables are integers and compared exactly; metrics are the same float64 arithmetic on the same integers (rtol 1e-12)."""
import os
import types

import numpy as np
import pytest
import torch

import insseg_ref as R

# the hook entries of configs/scannet/insseg-pointgroup-v1m1-0-spunet-base.py (segment_ignore_index = (-1, 0, 1) there),
# configs/_base_/default_runtime.py as configs/scannet/semseg-pt-v3m1-0-base.py inherits it, and the ModelNet40
# classification configs (configs/modelnet40/cls-spunet-v1m1-0-base.py lists it; cls-ptv3-v1m1-0-base.py has no
# evaluator entry in the reference tree)
CONFIG_HOOKS = [
    dict(type="InsSegEvaluator", segment_ignore_index=(-1, 0, 1), instance_ignore_index=-1),
    dict(type="SemSegEvaluator"),
    dict(type="ClsEvaluator"),
]
RTOL = 1e-12
SEM_RUNS = ["sem0", "sem1", "sem2", "sem3", "sem4"]


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return np.load(os.path.join(golden_dir, "seg_evaluators.npz"))


@pytest.fixture()
def cuda_is_identity(monkeypatch):
    monkeypatch.setattr(torch.Tensor, "cuda", lambda self, *a, **k: self)


def HOOKS_BUILD(cfg):
    from pointcept.engines.hooks.builder import HOOKS
    import pointcept.engines.hooks  # noqa: F401
    return HOOKS.build(cfg)


class _Model:
    def eval(self):
        return self

    def __call__(self, d):
        return dict(d["_out"])


def loader_of(g, tag, out_keys, device="cpu", out_device=None):
    """The run's batches as the hook's val_loader sees them; the model's outputs ride along in a dict under "_out", which
    the hook's move to the device leaves where it is."""
    out_device = out_device or device
    loader = []
    for i in range(int(g[tag + "_nbatch"])):
        pre = f"{tag}_b{i}_"
        b = {"_out": {}}
        for key in g.files:
            if not key.startswith(pre):
                continue
            name = key[len(pre):]
            if name == "name":
                b["name"] = [str(g[key])]
            elif name in out_keys:
                b["_out"][name] = torch.from_numpy(g[key]).to(out_device)
            elif name != "idx":
                b[name] = torch.from_numpy(g[key]).to(device)
        loader.append(b)
    return loader


def trainer_of(g, tag, loader, out_keys):
    k, ignore = int(g[tag + "_cfg"][0]), int(g[tag + "_cfg"][1])
    logs, scalars = [], {}
    trainer = types.SimpleNamespace(
        val_loader=loader, model=_Model(), logger=types.SimpleNamespace(info=logs.append),
        writer=types.SimpleNamespace(add_scalar=lambda key, v, e: scalars.__setitem__(key, v)), epoch=0, comm_info={},
        best_metric_value=0.0,
        cfg=types.SimpleNamespace(evaluate=True, enable_wandb=False, data=types.SimpleNamespace(
            num_classes=k, ignore_index=ignore, names=[f"c{i}" for i in range(k)])))
    return trainer, logs, scalars


def check_report(g, tag, trainer, logs, scalars):
    """Log lines, writer keys and values, comm_info against the fixture."""
    assert logs == str(g[tag + "_logs"]).split("\n")
    assert list(scalars) == str(g[tag + "_scalar_keys"]).split("\n")
    got = np.array([float(v) for v in scalars.values()])
    want = g[tag + "_scalar_values"]
    assert np.array_equal(np.isnan(got), np.isnan(want))
    print(tag, "largest relative difference", np.nanmax(np.abs(got - want) / np.abs(want)))
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=0)
    assert trainer.comm_info["current_metric_name"] == str(g[tag + "_metric_name"])
    np.testing.assert_allclose(trainer.comm_info["current_metric_value"], float(g[tag + "_metric_value"]), rtol=RTOL)


def run_seg_hook(g, tag, device="cpu"):
    cls = tag.startswith("cls")
    out_keys = ("cls_logits", "loss") if cls else ("seg_logits", "loss")
    trainer, logs, scalars = trainer_of(g, tag, loader_of(g, tag, out_keys, device), out_keys)
    hook = HOOKS_BUILD(dict(type="ClsEvaluator") if cls else
                       dict(type="SemSegEvaluator", write_cls_iou=bool(g[tag + "_cfg"][2])))
    hook.trainer = trainer
    hook.before_train()
    hook.after_epoch()
    hook.after_train()
    check_report(g, tag, trainer, logs, scalars)
    counts = hook.counts
    assert counts.dtype == np.int64
    assert np.array_equal(counts[0], g[tag + "_intersection"])
    assert np.array_equal(counts[1] + counts[2] - counts[0], g[tag + "_union"])
    assert np.array_equal(counts[2], g[tag + "_target"])
    return hook


def run_ins_hook(g, device="cpu", out_device=None, monkeypatch=None):
    import pointcept.engines.hooks.evaluator as E
    tag = "ins0"
    out_keys = ("pred_masks", "pred_classes", "pred_scores", "loss")
    loader = loader_of(g, tag, out_keys, device, out_device)
    by_size = {int(g[k].shape[0]): torch.from_numpy(g[k]) for k in g.files if k.startswith(tag) and k.endswith("_idx")}
    assert len(by_size) == 1   # one scene carries origin_coord

    def knn_query(k, coord, offset, new_coord, new_offset):   # the idx the fixture's run used: no kNN here
        return by_size[int(new_coord.shape[0])].view(-1, 1).int().to(new_coord.device), None

    monkeypatch.setattr(E.pointops, "knn_query", knn_query)
    trainer, logs, scalars = trainer_of(g, tag, loader, out_keys)
    hook = HOOKS_BUILD(dict(CONFIG_HOOKS[0], segment_ignore_index=tuple(g[tag + "_segment_ignore_index"].tolist())))
    hook.trainer = trainer
    hook.before_train()
    hook.after_epoch()
    check_report(g, tag, trainer, logs, scalars)
    hook.after_train()   # the reference's InsSegEvaluator leaves the closing line to HookBase's no-op
    assert logs[-1] == "Best AP50: 0.0000"
    check_ins_tables(g, hook)
    return hook


def check_ins_tables(g, hook):
    tag = "ins0"
    ignore = tuple(g[tag + "_segment_ignore_index"].tolist())
    scenes = list(hook.scenes.values())
    assert len(scenes) == int(g[tag + "_nbatch"])
    for si, scene in enumerate(scenes):
        kept = hook.kept_proposals(scene)
        assert np.array_equal(kept, g[f"{tag}_s{si}_kept"])
        assert np.array_equal(scene["vert_count"][kept], g[f"{tag}_s{si}_vert_count"])
        assert np.array_equal(scene["void_intersection"][kept], g[f"{tag}_s{si}_void_intersection"])
        assert np.array_equal(R.pairs(scene, scene["pred_classes"], ignore), g[f"{tag}_s{si}_pairs"])
        gt = np.stack([scene["gt_id"], scene["gt_class"], scene["gt_count"]], axis=1)
        want = g[f"{tag}_s{si}_gt"]
        assert np.array_equal(gt[np.argsort(gt[:, 0])], want[np.argsort(want[:, 0])])
        assert np.array_equal(scene["pred_scores"], g[f"{tag}_b{si}_pred_scores"].astype(np.float64))
    # the whole class x overlap table, nan where the reference has nan
    assert np.array_equal(hook.overlaps, g[tag + "_overlaps"])
    table = np.full(g[tag + "_ap_table"].shape, np.inf)
    for oi in range(len(hook.overlaps)):
        one = type(hook)(segment_ignore_index=ignore, instance_ignore_index=-1)
        one.trainer = hook.trainer
        one.before_train()
        one.overlaps = hook.overlaps[oi:oi + 1]
        with np.errstate(all="ignore"):
            import warnings
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                scores = one.evaluate_matches(scenes)
        key = "ap25%" if np.isclose(hook.overlaps[oi], 0.25) else "ap"
        table[:, oi] = [scores["classes"][n][key] for n in one.valid_class_names]
    want = g[tag + "_ap_table"]
    assert np.array_equal(np.isnan(table), np.isnan(want)) and np.isnan(want).any() and (want == 0).any()
    np.testing.assert_allclose(table, want, rtol=RTOL, atol=0)


def test_hooks_are_registered_and_build_from_the_config_entries():
    from pointcept.engines.hooks.builder import HOOKS, build_hooks
    import pointcept.engines.hooks  # noqa: F401
    hooks = build_hooks(CONFIG_HOOKS)
    assert [type(h).__name__ for h in hooks] == ["InsSegEvaluator", "SemSegEvaluator", "ClsEvaluator"]
    for h in hooks:
        assert HOOKS.get(type(h).__name__) is type(h)
    assert hooks[0].segment_ignore_index == (-1, 0, 1) and hooks[0].instance_ignore_index == -1
    assert hooks[1].write_cls_iou is False
    default = HOOKS.build(dict(type="InsSegEvaluator"))
    assert default.segment_ignore_index == (-1,) and default.min_region_sizes == 100
    assert np.allclose(default.overlaps, [0.5, 0.55, 0.6, 0.65, 0.7, 0.75, 0.8, 0.85, 0.9, 0.25])


@pytest.mark.parametrize("tag", SEM_RUNS + ["cls0"])
def test_semseg_and_cls_hooks_reproduce_the_reference(fixture, cuda_is_identity, tag):
    run_seg_hook(fixture, tag)


def test_insseg_hook_reproduces_the_reference(fixture, cuda_is_identity, monkeypatch):
    hook = run_ins_hook(fixture, monkeypatch=monkeypatch)
    # the hook's tables against the restatement that walks the labels pair by pair
    g, ignore = fixture, (-1, 0, 1)
    for si, scene in enumerate(hook.scenes.values()):
        pre = f"ins0_b{si}_"
        origin = pre + "idx" in g.files
        want = R.scene_tables(g[pre + "pred_masks"], g[pre + ("origin_segment" if origin else "segment")],
                              g[pre + ("origin_instance" if origin else "instance")], ignore, -1,
                              g[pre + "idx"] if origin else None)
        for key, value in want.items():
            assert np.array_equal(scene[key], value), key


def test_confusion_composition_and_numpy_functions_agree(fixture):
    """ops.seg_confusion_torch (what CPU tensors and K above the cap take), intersection_and_union and
    intersection_and_union_gpu against the bincount restatement; ties go to the lowest index."""
    from ptv3_hip import ops
    from pointcept.utils.misc import intersection_and_union, intersection_and_union_gpu
    g = fixture
    logits, segment = g["sem4_b0_seg_logits"], g["sem4_b0_segment"]
    pred = R.argmax_first(logits)
    assert (np.sort(logits, axis=1)[:, -1] == np.sort(logits, axis=1)[:, -2]).any()   # the fixture's rows do tie
    want = R.confusion(pred, segment, 13, -1)
    got = ops.seg_confusion_torch(torch.from_numpy(logits), torch.from_numpy(segment), 13, -1)
    assert got.dtype == torch.int64 and np.array_equal(got.numpy(), want)
    twice = ops.seg_confusion_torch(torch.from_numpy(pred), torch.from_numpy(segment).int(), 13, -1, counts=got)
    assert twice is got and np.array_equal(got.numpy(), 2 * want)
    i, u, t = intersection_and_union(pred, segment, 13, -1)
    assert np.array_equal(i, want[0]) and np.array_equal(u, want[1] + want[2] - want[0]) and np.array_equal(t, want[2])
    i, u, t = intersection_and_union_gpu(torch.from_numpy(pred.copy()), torch.from_numpy(segment), 13, -1)
    assert np.array_equal(i.numpy(), want[0]) and np.array_equal(u.numpy(), want[1] + want[2] - want[0])
    assert np.array_equal(t.numpy(), want[2])
    inv, origin = g["sem1_b0_inverse"], g["sem1_b0_origin_segment"]
    pred = R.argmax_first(g["sem1_b0_seg_logits"])
    got = ops.seg_confusion_torch(torch.from_numpy(g["sem1_b0_seg_logits"]), torch.from_numpy(origin), 13, -1,
                                  inverse=torch.from_numpy(inv))
    assert np.array_equal(got.numpy(), R.confusion(pred[inv], origin, 13, -1))


def test_ops_refuse_cpu_tensors():
    from ptv3_hip import ops
    with pytest.raises(RuntimeError, match="GPU tensor"):
        ops.seg_confusion(torch.zeros(4, 3), torch.zeros(4, dtype=torch.int64), 3)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        ops.insseg_associate(torch.zeros(2, 4, dtype=torch.int32), torch.zeros(4, dtype=torch.int32), 1)


def test_entry_points_validate_before_any_launch():
    import importlib
    L = importlib.import_module("ptv3_hip.lib")   # the module: ptv3_hip.lib, the attribute, is its handle object
    lib = L.lib
    assert L.PTV3_SEG_CONFUSION_MAX_K >= 200 and L.PTV3_INSSEG_MAX_GT >= 300 and lib.ptv3_insseg_chunk() > 0
    rc = lib.ptv3_seg_confusion(None, L.PTV3_F32, 4, None, None, L.PTV3_I64, 4, L.PTV3_SEG_CONFUSION_MAX_K + 1, -1, None,
                                None, None)
    assert rc != 0 and b"unsupported" in lib.ptv3_last_error()
    rc = lib.ptv3_seg_confusion(None, L.PTV3_F32, 4, None, None, L.PTV3_I64, 5, 3, -1, None, None, None)
    assert rc != 0 and b"no inverse" in lib.ptv3_last_error()
    rc = lib.ptv3_insseg_associate(None, L.PTV3_F32, 1, 4, None, None, 4, 2, None, None, None, None)
    assert rc != 0 and b"mask dtype" in lib.ptv3_last_error()
    rc = lib.ptv3_insseg_associate(None, L.PTV3_I32, 1, 4, None, None, 4, L.PTV3_INSSEG_MAX_GT + 1, None, None, None, None)
    assert rc != 0 and b"unsupported" in lib.ptv3_last_error()
    rc = lib.ptv3_insseg_associate(None, L.PTV3_I32, 1, 4, None, None, 5, 2, None, None, None, None)
    assert rc != 0 and b"no col_start" in lib.ptv3_last_error()
    assert lib.ptv3_insseg_associate(None, L.PTV3_I32, 0, 4, None, None, 4, 2, None, None, None, None) == 0


def test_comm_gather_at_world_size_one():
    from pointcept.utils import comm
    data = {"scene": np.arange(3)}
    out = comm.gather(data, dst=0)
    assert isinstance(out, list) and len(out) == 1 and out[0] is data
    assert comm.gather(5) == [5]


def test_pointgroup_device_results_default_off(monkeypatch):
    """set_device_results is opt-in: by default the proposals come back as CPU tensors, exactly what pg_proposals made."""
    from pointcept.models.point_group import point_group_v1m1_base as M
    model = types.SimpleNamespace(_device_results=False, voxel_size=0.02, segment_ignore_index=(-1, 0, 1),
                                  cluster_propose_points=100)
    assert M.PointGroupBase.set_device_results(model) is model and model._device_results is True
    assert M.PointGroupBase.set_device_results(model, False)._device_results is False
    made = (torch.tensor([2, 3]), torch.tensor([0.5, 0.25]), torch.ones((2, 6), dtype=torch.int32))
    moved = []

    class Tracked(torch.Tensor):
        def cpu(self):
            moved.append(1)
            return torch.Tensor.cpu(self).as_subclass(torch.Tensor)

    monkeypatch.setattr(M.ops, "pg_proposals", lambda *a, **k: tuple(t.as_subclass(Tracked) for t in made))
    model.cluster = lambda center, seg, keep, offset: (torch.zeros((0, 2)), torch.zeros(1), torch.arange(6), 2)
    args = (torch.rand(6, 3), torch.rand(6, 3), torch.rand(6, 4) + torch.tensor([0, 0, 5.0, 0]), torch.tensor([6]))
    off = M.PointGroupBase._proposals(model, *args)
    assert len(moved) == 3 and sorted(off) == ["pred_classes", "pred_masks", "pred_scores"]
    assert torch.equal(off["pred_classes"], made[0]) and torch.equal(off["pred_scores"], made[1])
    assert torch.equal(off["pred_masks"], made[2])
    model._device_results = True
    on = M.PointGroupBase._proposals(model, *args)
    assert len(moved) == 3 and torch.equal(on["pred_masks"], made[2])   # nothing copied
    import inspect
    assert inspect.signature(M.PointGroupBase.set_device_results).parameters["on"].default is True
    assert "_device_results = False" in inspect.getsource(M.PointGroupBase.__init__)
