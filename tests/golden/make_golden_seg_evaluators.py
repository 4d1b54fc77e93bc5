"""tests/golden/seg_evaluators.npz: the reference's ClsEvaluator, SemSegEvaluator and InsSegEvaluator hooks
(engines/hooks/evaluator.py:22-645) run on seeded batches, imported in place from the reference tree (ref_loader.REF).

    python tests/golden/make_golden_seg_evaluators.py

The hook file, utils/misc.py and utils/comm.py are imported where they lie, through ref_loader's bare `pointcept`
packages.  What a machine without a GPU lacks is shimmed HERE, on top of ref_loader.load(), never in the hooks:
  * `wandb` and `pointops` are bare modules; pointops.knn_query is a brute-force nearest neighbour, and the `idx` it
    returned is stored so that no test needs a kNN;
  * `Tensor.cuda` is the identity (the generator runs without a GPU);
  * the trainer is a stub: model = a callable returning stored outputs, val_loader = the list of batches, logger / writer /
    storage record what the hook reports (storage restates the running total / count / avg of utils/events.py:511-530);
  * CPU torch has no integer histc ("histogram_cpu" not implemented for 'Long'), so the hook's intersection_and_union_gpu
    is wrapped with a float64 cast of its two inputs.  Counts stay exact far below 2^53.
Stored per run: the inputs and everything the hook reported (log lines, writer scalars, comm_info, the summed areas; for
insseg the per-class AP table and, per scene and kept proposal, vert_count, void_intersection and the (ground-truth
instance id, intersection) pairs).  The insseg run asserts that the reference took every branch worth pinning.
"""
import collections
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import ref_loader  # noqa: E402


class Meter:
    def __init__(self):
        self.total, self.count, self.avg = 0, 0, 0

    def update(self, val, n=1):
        self.total += val * n
        self.count += n
        self.avg = self.total / self.count


class Storage:
    def __init__(self):
        self.h = collections.defaultdict(Meter)

    def put_scalar(self, name, value, n=1, smoothing_hint=False):
        self.h[name].update(value, n)

    def history(self, name):
        return self.h[name]


class Model:
    def eval(self):
        return self

    def __call__(self, d):
        return dict(d["_out"])


def trainer_for(loader, num_classes, ignore_index):
    logs, scalars = [], {}
    t = types.SimpleNamespace(
        val_loader=[dict(b) for b in loader], model=Model(), logger=types.SimpleNamespace(info=logs.append),
        writer=types.SimpleNamespace(add_scalar=lambda k, v, e: scalars.__setitem__(k, v)), epoch=0, comm_info={},
        storage=Storage(), best_metric_value=0.0,
        cfg=types.SimpleNamespace(evaluate=True, enable_wandb=False, data=types.SimpleNamespace(
            num_classes=num_classes, ignore_index=ignore_index, names=[f"c{i}" for i in range(num_classes)])))
    return t, logs, scalars


def seg_batch(seed, n, k, ignore, n_origin=0, absent=None, beyond=False):
    g = torch.Generator().manual_seed(seed)
    segment = torch.randint(0, k, (n,), generator=g)
    if absent is not None:                                   # a class that never occurs, as target or as prediction
        segment[segment == absent] = (absent + 1) % k
    logits = (torch.randn(n, k, generator=g) * 8).round() / 8   # eighths: exact in bf16 / fp16 too, and rows tie
    logits[torch.arange(n), segment] += 1.5                  # often right
    if absent is not None:
        logits[:, absent] = -9.0
    segment[torch.rand(n, generator=g) < 0.1] = ignore
    if beyond:                                               # target values >= K that are not the ignore index
        segment[torch.rand(n, generator=g) < 0.05] = k + 3
    d = dict(segment=segment, offset=torch.tensor([n]),
             _out=dict(seg_logits=logits, loss=torch.rand((), generator=g) + 0.5))
    if n_origin:
        inverse = torch.randint(0, n, (n_origin,), generator=g)
        origin = segment[inverse].clone()
        flip = torch.rand(n_origin, generator=g) < 0.1
        origin[flip] = torch.randint(-1, k, (int(flip.sum()),), generator=g).clamp(min=0)
        origin[torch.rand(n_origin, generator=g) < 0.05] = ignore
        # of origin_coord the hook reads only its presence
        d.update(inverse=inverse, origin_segment=origin, origin_coord=torch.zeros(n_origin, 3))
    return d


def cls_batch(seed, b, k):
    g = torch.Generator().manual_seed(seed)
    category = torch.randint(0, k, (b,), generator=g)
    logits = torch.randn(b, k, generator=g)
    logits[torch.arange(b), category] += 2.0
    return dict(category=category, offset=torch.arange(1, b + 1) * 10,
                _out=dict(cls_logits=logits, loss=torch.rand((), generator=g) + 0.5))


INS_CLASSES, INS_IGNORE = 7, (-1, 0, 1)


def ins_scene(seed, name, with_origin=False):
    """About 2 500 points in runs of one instance each; proposals are shifted and stretched runs.  Class 5 has ground
    truth and never a proposal, class 6 has neither."""
    g = torch.Generator().manual_seed(seed)

    def rnd(lo, hi):
        return int(torch.randint(lo, hi, (1,), generator=g))

    runs = []   # (length, segment, instance id or -1)
    runs.append((rnd(150, 250), 0, -1))                       # floor: void, no instance
    runs.append((rnd(120, 200), 1, 100))                      # wall: an instance of an ignored segment
    classes = [2, 2, 3, 3, 4, 4, 2, 3, 5, 4, 2, 3]
    for i, c in enumerate(classes):
        runs.append((rnd(120, 260), c, 7 + 3 * i))
    runs.append((rnd(40, 90), 4, 3))                          # a ground truth under 100 points
    runs.append((rnd(40, 90), 2, 5))                          # and another
    runs.append((rnd(100, 160), -1, -1))                      # unlabelled
    segment = torch.cat([torch.full((l,), s) for l, s, _ in runs])
    instance = torch.cat([torch.full((l,), i) for l, _, i in runs])
    n = segment.shape[0]
    starts = np.cumsum([0] + [l for l, _, _ in runs])
    masks, classes_p = [], []

    def propose(a, b, c, value=1):
        m = torch.zeros(n, dtype=torch.int32)
        m[max(a, 0):min(b, n)] = value
        masks.append(m)
        classes_p.append(c)

    for r, (l, s, i) in enumerate(runs):
        a, b = int(starts[r]), int(starts[r + 1])
        if s in (2, 3, 4) and l >= 100:
            # one or two proposals per instance, IoU from about 0.2 to 0.95
            shift = rnd(-l // 2, l // 2) if r % 3 else rnd(-l // 12, l // 12)
            propose(a + shift, b + shift + rnd(-l // 6, l // 6), s, value=(2 if r % 4 == 0 else 1))
            if r % 2 == 0:
                propose(a + rnd(0, l // 10), b - rnd(0, l // 10), s, value=(-1 if r % 4 == 2 else 1))   # the duplicate
        if s == 4 and l < 100:
            propose(a - 30, b + 40, 4)                        # mostly on a small ground truth and its neighbours
    propose(0, int(starts[1]) - 10, 2)                        # on the floor: void, dropped as ignored
    propose(int(starts[1]) - 60, int(starts[1]) + 70, 3)      # half void, half wall: kept as a false positive at 0.5
    propose(int(starts[2]) + 10, int(starts[2]) + 70, 2)      # under 100 points
    propose(int(starts[3]), int(starts[4]), 0)                # an ignored class
    propose(int(starts[3]), int(starts[4]), 1)
    propose(int(starts[-2]) - 20, n, 4)                       # on unlabelled points (void): dropped
    propose(int(starts[5]) + 5, int(starts[6]) - 5, 3 if runs[5][1] != 3 else 2)   # right place, wrong class
    p = len(masks)
    order = torch.randperm(p, generator=g)
    masks = torch.stack(masks)[order]
    classes_p = torch.tensor(classes_p)[order]
    scores = torch.rand(p, generator=g)
    d = dict(name=[name], coord=torch.rand(n, 3, generator=g) * 4, segment=segment, instance=instance,
             offset=torch.tensor([n]),
             _out=dict(pred_masks=masks, pred_classes=classes_p, pred_scores=scores,
                       loss=torch.rand((), generator=g) + 0.5))
    if with_origin:
        n_origin = n + n * 3 // 5
        origin_coord = torch.rand(n_origin, 3, generator=g) * 4
        idx = torch.cdist(origin_coord, d["coord"]).argmin(1)
        d.update(origin_coord=origin_coord, origin_offset=torch.tensor([n_origin]), origin_segment=segment[idx].clone(),
                 origin_instance=instance[idx].clone(), _idx=idx)
    return d


def store_batches(out, tag, loader):
    out[tag + "_nbatch"] = np.array(len(loader))
    for i, b in enumerate(loader):
        for k, v in b.items():
            if k == "_out":
                for k2, v2 in v.items():
                    out[f"{tag}_b{i}_{k2}"] = v2.numpy()
            elif k == "name":
                out[f"{tag}_b{i}_name"] = np.array(v[0])
            else:
                out[f"{tag}_b{i}_{k.lstrip('_')}"] = v.numpy()


def store_report(out, tag, trainer, logs, scalars):
    out[tag + "_logs"] = np.array("\n".join(logs))
    out[tag + "_scalar_keys"] = np.array("\n".join(scalars))
    out[tag + "_scalar_values"] = np.array([float(v) for v in scalars.values()], dtype=np.float64)
    out[tag + "_metric_value"] = np.array(trainer.comm_info["current_metric_value"], dtype=np.float64)
    out[tag + "_metric_name"] = np.array(trainer.comm_info["current_metric_name"])


def main():
    ref_loader.load()
    for name in ("wandb", "pointops"):
        sys.modules[name] = types.ModuleType(name)
    hooks_pkg = sys.modules["pointcept.engines.hooks"]
    default = importlib.import_module("pointcept.engines.hooks.default")
    hooks_pkg.HookBase = default.HookBase
    ev = importlib.import_module("pointcept.engines.hooks.evaluator")
    torch.Tensor.cuda = lambda self, *a, **k: self      # the generator runs without a GPU
    reference_iou = ev.intersection_and_union_gpu
    ev.intersection_and_union_gpu = lambda o, t, k, i=-1: reference_iou(o.double(), t.double(), k, i)
    out = {}

    # ---- semseg ------------------------------------------------------------------------------------------------
    sem_runs = [
        ("sem0", 13, -1, [seg_batch(1, 3001, 13, -1), seg_batch(2, 2950, 13, -1)], False),
        ("sem1", 13, -1, [seg_batch(3, 3010, 13, -1, n_origin=5003), seg_batch(4, 2999, 13, -1, n_origin=4900)], True),
        ("sem2", 2, 255, [seg_batch(5, 3000, 2, 255), seg_batch(6, 2800, 2, 255)], False),
        ("sem3", 13, -1, [seg_batch(7, 3000, 13, -1, absent=4), seg_batch(8, 3100, 13, -1, absent=4)], False),
        ("sem4", 13, -1, [seg_batch(9, 3000, 13, -1, beyond=True), seg_batch(10, 2900, 13, -1, beyond=True)], True),
    ]
    for tag, k, ignore, loader, write_cls_iou in sem_runs:
        trainer, logs, scalars = trainer_for(loader, k, ignore)
        hook = ev.SemSegEvaluator(write_cls_iou=write_cls_iou)
        hook.trainer = trainer
        hook.after_epoch()
        hook.after_train()
        store_batches(out, tag, loader)
        store_report(out, tag, trainer, logs, scalars)
        out[tag + "_cfg"] = np.array([k, ignore, int(write_cls_iou)])
        for key in ("intersection", "union", "target"):
            out[f"{tag}_{key}"] = np.asarray(trainer.storage.history("val_" + key).total).astype(np.int64)
        if tag == "sem3":
            assert out[tag + "_target"][4] == 0 and out[tag + "_union"][4] == 0
        if tag == "sem4":
            assert any((b["segment"] == 16).any() for b in loader)
        print(tag, scalars["val/mIoU"], scalars["val/allAcc"])

    # ---- cls ---------------------------------------------------------------------------------------------------
    loader = [cls_batch(11, 8, 40), cls_batch(12, 5, 40)]
    trainer, logs, scalars = trainer_for(loader, 40, -1)
    hook = ev.ClsEvaluator()
    hook.trainer = trainer
    hook.after_epoch()
    hook.after_train()
    store_batches(out, "cls0", loader)
    store_report(out, "cls0", trainer, logs, scalars)
    out["cls0_cfg"] = np.array([40, -1, 0])
    for key in ("intersection", "union", "target"):
        out[f"cls0_{key}"] = np.asarray(trainer.storage.history("val_" + key).total).astype(np.int64)
    print("cls0", scalars["val/allAcc"])

    # ---- insseg ------------------------------------------------------------------------------------------------
    loader = [ins_scene(21, "scene_a"), ins_scene(22, "scene_b", with_origin=True), ins_scene(23, "scene_c")]
    by_offset = {int(b["origin_offset"][0]): b["_idx"] for b in loader if "_idx" in b}
    sys.modules["pointops"].knn_query = lambda k, c, o, oc, oo: (by_offset[int(oo[0])].view(-1, 1).int(), None)
    ev.pointops = sys.modules["pointops"]
    trainer, logs, scalars = trainer_for(loader, INS_CLASSES, -1)
    hook = ev.InsSegEvaluator(segment_ignore_index=INS_IGNORE, instance_ignore_index=-1)
    hook.trainer = trainer
    hook.before_train()
    recorded = []
    associate = hook.associate_instances

    def recording(pred, segment, instance):
        gt, pr = associate(pred, segment, instance)
        recorded.append((gt, pr, pred, segment.numpy(), instance.numpy()))
        return gt, pr

    hook.associate_instances = recording
    tables = []
    evaluate = hook.evaluate_matches

    def recording_matches(scenes):
        # the class x overlap table is a local of evaluate_matches: rebuild it from per-overlap calls
        scores = evaluate(scenes)
        overlaps = hook.overlaps
        table = np.zeros((len(hook.valid_class_names), len(overlaps)))
        for oi in range(len(overlaps)):
            hook.overlaps = overlaps[oi:oi + 1]
            one = evaluate(scenes)
            # a single overlap is "all but 0.25" or "0.25": its per-class value sits under one of the two keys
            key = "ap25%" if np.isclose(overlaps[oi], 0.25) else "ap"
            table[:, oi] = [one["classes"][n][key] for n in hook.valid_class_names]
        hook.overlaps = overlaps
        tables.append(table)
        return scores

    hook.evaluate_matches = recording_matches
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        hook.after_epoch()
    store_batches(out, "ins0", loader)
    store_report(out, "ins0", trainer, logs, scalars)
    out["ins0_cfg"] = np.array([INS_CLASSES, -1, 0])
    out["ins0_segment_ignore_index"] = np.array(INS_IGNORE)
    out["ins0_ap_table"] = tables[0]                                    # (valid classes, overlaps)
    out["ins0_overlaps"] = hook.overlaps
    names = hook.valid_class_names
    # per-class AP / AP50 / AP25 as the hook logged them come from this table; the three means are in the scalars
    took = collections.Counter()
    for si, (gt, pr, pred, segment, instance) in enumerate(recorded):
        kept = sorted((p for n in names for p in pr[n]), key=lambda p: p["instance_id"])
        # which proposal each kept one is: replay the two filters of :310 / :322 over the raw proposals
        masks = pred["pred_masks"].numpy()
        raw = [i for i in range(masks.shape[0]) if int(pred["pred_classes"][i]) not in INS_IGNORE
               and np.count_nonzero(masks[i]) >= 100]
        assert len(raw) == len(kept)
        pairs = [(k, int(g["instance_id"]), int(g["intersection"])) for k, p in enumerate(kept) for g in p["matched_gt"]]
        out[f"ins0_s{si}_kept"] = np.array(raw)
        out[f"ins0_s{si}_vert_count"] = np.array([int(p["vert_count"]) for p in kept])
        out[f"ins0_s{si}_void_intersection"] = np.array([int(p["void_intersection"]) for p in kept])
        out[f"ins0_s{si}_pairs"] = np.array(pairs, dtype=np.int64).reshape(-1, 3)   # (kept proposal, gt id, intersection)
        out[f"ins0_s{si}_gt"] = np.array([(int(g["instance_id"]), int(g["segment_id"]), int(g["vert_count"]))
                                          for n in names for g in gt[n]], dtype=np.int64).reshape(-1, 3)
        # the branches the fixture is there to pin, at overlap 0.5
        took["mask_values"] += int(np.isin(masks, (0, 1), invert=True).any())
        took["small_proposal"] += sum(0 < np.count_nonzero(m) < 100 for m in masks)
        took["ignored_class_proposal"] += sum(int(c) in INS_IGNORE for c in pred["pred_classes"])
        for n in names:
            for g in gt[n]:
                took["small_gt"] += int(g["vert_count"] < 100)
                good = [p for p in g["matched_pred"] if g["vert_count"] >= 100 and
                        p["intersection"] / (g["vert_count"] + p["vert_count"] - p["intersection"]) > 0.5]
                took["duplicate_match"] += int(len(good) >= 2)
            for p in pr[n]:
                ious = [g["intersection"] / (g["vert_count"] + p["vert_count"] - g["intersection"])
                        for g in p["matched_gt"]]
                if not any(v > 0.5 for v in ious):
                    ignore = p["void_intersection"] + sum(g["intersection"] for g in p["matched_gt"]
                                                          if g["vert_count"] < 100)
                    took["unmatched_dropped" if ignore / p["vert_count"] > 0.5 else "unmatched_kept"] += 1
                took["iou_low"] += sum(0.2 < v < 0.5 for v in ious)
                took["iou_high"] += sum(v > 0.9 for v in ious)
    table = tables[0]
    o50 = int(np.flatnonzero(np.isclose(hook.overlaps, 0.5))[0])
    took["gt_without_prediction"] = int(table[names.index("c5"), o50] == 0.0)
    took["neither"] = int(np.isnan(table[names.index("c6"), o50]))
    print(dict(took))
    for key in ("mask_values", "small_proposal", "ignored_class_proposal", "small_gt", "duplicate_match",
                "unmatched_dropped", "unmatched_kept", "iou_low", "iou_high", "gt_without_prediction", "neither"):
        assert took[key] > 0, f"the reference never took the branch '{key}'"
    print("ins0", scalars, "\n", np.round(table, 3))
    path = os.path.join(HERE, "seg_evaluators.npz")
    np.savez_compressed(path, **out)
    print("seg_evaluators.npz", os.path.getsize(path))


if __name__ == "__main__":
    main()
