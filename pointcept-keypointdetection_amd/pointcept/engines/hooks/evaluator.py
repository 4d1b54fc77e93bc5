"""ClsEvaluator, SemSegEvaluator and InsSegEvaluator on the HIP path: hook names, constructor keywords, log lines, writer
keys and comm_info of the reference (pointcept/engines/hooks/evaluator.py:22-645).

Semseg / cls: the reference makes, per batch, an argmax, a gather, a masked write, a compaction, three histc calls, three
all-reduces, three copies to the host and an `.item()`.  Here a batch is one call that adds to a (3, K) table on the
device (pointcept.utils.misc.confusion_counts), the losses stay there too, and an epoch ends with one all-reduce and one
host read.  The per-batch "Test: [i/n] Loss" lines are kept and printed from that one read, after the last batch.

Insseg: associate_instances (:269-342) makes one pass over the scene per (proposal, ground-truth instance) on the host.
Here the instance ids become a per-point code on the device (insseg_codes), ops.insseg_associate counts every proposal
against every instance in one launch - reading the masks through the nearest-neighbour map instead of gathering them
(:577) - and one copy brings the small tables to the host, where evaluate_matches (:344-546) is restated over arrays in
float64.  Ranks gather those tables, not dicts of masks.  A model with set_device_results (PointGroup) keeps its
proposals on the device for the evaluation.
"""
import numpy as np
import torch
import torch.distributed as dist

import pointops
import pointcept.utils.comm as comm
from pointcept.utils.misc import confusion_counts
from pointcept.engines.hooks.builder import HOOKS
from pointcept.engines.hooks import HookBase
from ptv3_hip import ops


def _wandb():
    import wandb   # optional: only a run with cfg.enable_wandb needs it
    return wandb


def _to_device(input_dict):
    for key in input_dict.keys():
        if isinstance(input_dict[key], torch.Tensor):
            input_dict[key] = input_dict[key].cuda(non_blocking=True)


def _read_epoch(counts, losses):
    """The one host read: (counts as an integer array or None, the batch losses as Python floats)."""
    parts = [torch.stack([l.detach().double().reshape(()) for l in losses])] if losses else []
    if counts is not None:
        parts.insert(0, counts.reshape(-1).double())   # exact below 2^53
    if not parts:
        return None, []
    host = torch.cat(parts).cpu().numpy()
    if counts is None:
        return None, host.tolist()
    return host[: counts.numel()].astype(np.int64).reshape(counts.shape), host[counts.numel():].tolist()


def _mean(values):
    """AverageMeter.avg of utils/events.py:526-530 over the values in order."""
    total = 0
    for v in values:
        total += v
    return total / len(values)


class _SegCountEvaluator(HookBase):
    """What ClsEvaluator and SemSegEvaluator share: the (3, K) table of an epoch and what is reported from it."""
    metric_name = None

    def after_epoch(self):
        if self.trainer.cfg.evaluate:
            self.eval()

    def _batch(self, input_dict, output_dict):
        """(logits, target, inverse or None, prefix of the batch's log line)"""
        raise NotImplementedError

    def eval(self):
        trainer = self.trainer
        trainer.logger.info(">>>>>>>>>>>>>>>> Start Evaluation >>>>>>>>>>>>>>>>")
        trainer.model.eval()
        num_classes = trainer.cfg.data.num_classes
        counts, losses, prefixes = None, [], []
        for input_dict in trainer.val_loader:
            _to_device(input_dict)
            with torch.no_grad():
                output_dict = trainer.model(input_dict)
            logits, target, inverse, prefix = self._batch(input_dict, output_dict)
            counts = confusion_counts(logits, target, num_classes, trainer.cfg.data.ignore_index, inverse, counts)
            losses.append(output_dict["loss"])
            prefixes.append(prefix)
        if counts is not None and comm.get_world_size() > 1:
            dist.all_reduce(counts)
        counts, losses = _read_epoch(counts, losses)
        for i, (prefix, loss) in enumerate(zip(prefixes, losses)):
            trainer.logger.info(prefix + "Test: [{iter}/{max_iter}] ".format(iter=i + 1, max_iter=len(prefixes))
                                + "Loss {loss:.4f} ".format(loss=loss))
        self.counts = counts                         # (3, K) int64 of this evaluation
        intersection, target = counts[0], counts[2]
        union = counts[1] + counts[2] - counts[0]
        loss_avg = _mean(losses)
        iou_class = intersection / (union + 1e-10)
        acc_class = intersection / (target + 1e-10)
        m_iou = np.mean(iou_class)
        m_acc = np.mean(acc_class)
        all_acc = sum(intersection) / (sum(target) + 1e-10)
        trainer.logger.info("Val result: mIoU/mAcc/allAcc {:.4f}/{:.4f}/{:.4f}.".format(m_iou, m_acc, all_acc))
        for i in range(num_classes):
            trainer.logger.info("Class_{idx}-{name} Result: iou/accuracy {iou:.4f}/{accuracy:.4f}".format(
                idx=i, name=trainer.cfg.data.names[i], iou=iou_class[i], accuracy=acc_class[i]))
        current_epoch = trainer.epoch + 1
        if trainer.writer is not None:
            scalars = {"val/loss": loss_avg, "val/mIoU": m_iou, "val/mAcc": m_acc, "val/allAcc": all_acc}
            for key, value in scalars.items():
                trainer.writer.add_scalar(key, value, current_epoch)
            if trainer.cfg.enable_wandb:
                wandb = _wandb()
                wandb.log({"Epoch": current_epoch, **scalars}, step=wandb.run.step)
            if getattr(self, "write_cls_iou", False):
                for i in range(num_classes):
                    key = f"val/cls_{i}-{trainer.cfg.data.names[i]} IoU"
                    trainer.writer.add_scalar(key, iou_class[i], current_epoch)
                    if trainer.cfg.enable_wandb:
                        wandb = _wandb()
                        wandb.log({"Epoch": current_epoch, key: iou_class[i]}, step=wandb.run.step)
        trainer.logger.info("<<<<<<<<<<<<<<<<< End Evaluation <<<<<<<<<<<<<<<<<")
        metric = {"mIoU": m_iou, "allAcc": all_acc}[self.metric_name]
        trainer.comm_info["current_metric_value"] = metric             # save for saver
        trainer.comm_info["current_metric_name"] = self.metric_name    # save for saver

    def after_train(self):
        self.trainer.logger.info("Best {}: {:.4f}".format(self.metric_name, self.trainer.best_metric_value))


@HOOKS.register_module()
class ClsEvaluator(_SegCountEvaluator):
    metric_name = "allAcc"

    def _batch(self, input_dict, output_dict):
        return output_dict["cls_logits"], input_dict["category"], None, ""


@HOOKS.register_module()
class SemSegEvaluator(_SegCountEvaluator):
    metric_name = "mIoU"

    def __init__(self, write_cls_iou=False):
        self.write_cls_iou = write_cls_iou

    def before_train(self):
        if self.trainer.writer is not None and self.trainer.cfg.enable_wandb:
            _wandb().define_metric("val/*", step_metric="Epoch")

    def _batch(self, input_dict, output_dict):
        segment, inverse = input_dict["segment"], None
        if "inverse" in input_dict.keys():
            assert "origin_segment" in input_dict.keys()
            segment, inverse = input_dict["origin_segment"], input_dict["inverse"]
        return (output_dict["seg_logits"], segment, inverse,
                "Interp. " if "origin_coord" in input_dict.keys() else "")


# ---- instance segmentation ----------------------------------------------------------------------------------------
# Shapes at which ptv3_insseg_associate measured ahead of the better of its two torch compositions by more than the
# run-to-run spread (tools/bench_evaluator.py): every shape timed, 100 to 800 proposals on 20 000
# to 240 000 evaluated points.  Fewer proposals or points were not timed and take the composition.
INSSEG_MIN_PROPOSALS = 100
INSSEG_MIN_POINTS = 20_000


def insseg_associate_wired(num_proposals, num_points, num_gt):
    return (num_proposals >= INSSEG_MIN_PROPOSALS and num_points >= INSSEG_MIN_POINTS
            and num_gt <= ops.INSSEG_MAX_GT)


def insseg_codes(segment, instance, segment_ignore_index, instance_ignore_index):
    """np.unique(instance, return_index, return_counts) and the two `continue`s of :285-293 in torch, on the inputs'
    device -> (code (N) int32 for ops.insseg_associate, G, gt_id (G), gt_class (G) = the segment at an instance's first
    point, gt_count (G)); the instances in ascending id, as np.unique lists them."""
    n = instance.shape[0]
    dev = instance.device
    ids, inv, cnt = torch.unique(instance, return_inverse=True, return_counts=True)
    first = torch.full_like(ids, n, dtype=torch.int64).scatter_reduce_(
        0, inv, torch.arange(n, device=dev), "amin", include_self=True)
    seg_ids = segment[first]
    ignored = torch.tensor(list(segment_ignore_index), device=dev, dtype=segment.dtype)
    keep = (ids != instance_ignore_index) & ~torch.isin(seg_ids, ignored)
    g = int(keep.sum())   # the width of the table: a host read
    compact = torch.where(keep, keep.cumsum(0) - 1, g)
    code = compact[inv].to(torch.int32)
    code = torch.where(torch.isin(segment, ignored), code + ops.INSSEG_VOID, code)
    return code, g, ids[keep], seg_ids[keep], cnt[keep]


def average_precision(y_true, y_score, hard_false_negatives):
    """Area under the precision-recall curve of :466-519: one point per distinct score, the [-0.5, 0, 0.5] steps."""
    order = np.argsort(y_score)
    score_sorted, true_sorted = y_score[order], y_true[order]
    true_cumsum = np.cumsum(true_sorted)
    _, first = np.unique(score_sorted, return_index=True)
    num_examples = len(score_sorted)
    num_true = true_cumsum[-1] if len(true_cumsum) > 0 else 0
    true_cumsum = np.append(true_cumsum, 0)        # index -1: nothing below the lowest score
    precision = np.zeros(len(first) + 1)
    recall = np.zeros(len(first) + 1)
    for k, j in enumerate(first):
        below = true_cumsum[j - 1]
        tp = num_true - below
        fp = num_examples - j - tp
        fn = below + hard_false_negatives
        precision[k] = float(tp) / (tp + fp)
        recall[k] = float(tp) / (tp + fn)
    precision[-1], recall[-1] = 1.0, 0.0           # the curve's artificial first point
    padded = np.append(np.append(recall[0], recall), 0.0)
    return np.dot(precision, np.convolve(padded, [-0.5, 0, 0.5], "valid"))


@HOOKS.register_module()
class InsSegEvaluator(HookBase):
    def __init__(self, segment_ignore_index=(-1,), instance_ignore_index=-1):
        self.segment_ignore_index = segment_ignore_index
        self.instance_ignore_index = instance_ignore_index

        self.valid_class_names = None  # update in before train
        self.valid_class_ids = None
        self.overlaps = np.append(np.arange(0.5, 0.95, 0.05), 0.25)
        self.min_region_sizes = 100
        self.distance_threshes = float("inf")
        self.distance_confs = -float("inf")

    def before_train(self):
        self.valid_class_ids = [i for i in range(self.trainer.cfg.data.num_classes)
                                if i not in self.segment_ignore_index]
        self.valid_class_names = [self.trainer.cfg.data.names[i] for i in self.valid_class_ids]

    def after_epoch(self):
        if self.trainer.cfg.evaluate:
            self.eval()

    def associate_instances(self, pred, segment, instance, idx=None):
        """One scene as compact host arrays: inter (P, G), vert_count (P), void_intersection (P), pred_classes (P),
        pred_scores (P) float64, gt_id / gt_class / gt_count (G).  Proposals are not filtered here; evaluate_matches
        drops the ignored classes and the small ones.  idx (N) maps the evaluated cloud to the masks' columns."""
        masks, classes, scores = pred["pred_masks"], pred["pred_classes"], pred["pred_scores"]
        assert classes.shape[0] == scores.shape[0] == masks.shape[0]
        dev = masks.device
        segment, instance = segment.to(dev), instance.to(dev)
        idx = None if idx is None else idx.to(dev)
        assert (masks.shape[1] if idx is None else idx.shape[0]) == segment.shape[0] == instance.shape[0]
        code, g, gt_id, gt_class, gt_count = insseg_codes(segment, instance, self.segment_ignore_index,
                                                          self.instance_ignore_index)
        p = masks.shape[0]
        if masks.is_cuda and insseg_associate_wired(p, code.shape[0], g):
            inter, vert, void = ops.insseg_associate(masks.contiguous(), code, g,
                                                     None if idx is None else idx.contiguous())
        else:
            inter, vert, void = ops.insseg_associate_torch(masks, code, g, idx)
        # one copy: the integer tables, then the scores as their bits
        packed = torch.cat([inter[:, :g].reshape(-1).long(), vert.long(), void.long(), classes.to(dev).long(),
                            scores.to(dev).float().contiguous().view(torch.int32).long(), gt_id.long(), gt_class.long(),
                            gt_count.long()]).cpu().numpy()
        sizes = [p * g, p, p, p, p, g, g, g]
        inter, vert, void, classes, scores, gt_id, gt_class, gt_count = np.split(packed, np.cumsum(sizes)[:-1])
        return dict(inter=inter.reshape(p, g), vert_count=vert, void_intersection=void, pred_classes=classes,
                    pred_scores=scores.astype(np.int32).view(np.float32).astype(np.float64), gt_id=gt_id,
                    gt_class=gt_class, gt_count=gt_count)

    def kept_proposals(self, scene, class_id=None):
        """Proposals that :310 and :322 keep, in their order, of one class or of every evaluated one."""
        ok = scene["vert_count"] >= self.min_region_sizes
        if class_id is None:
            ok &= ~np.isin(scene["pred_classes"], list(self.segment_ignore_index))
        else:
            ok &= scene["pred_classes"] == class_id
        return np.flatnonzero(ok)

    def _match_scene(self, scene, class_id, overlap_th):
        """(y_true, y_score, hard false negatives, has_gt, has_pred) of one scene, class and threshold (:371-457)."""
        inter, vert, score = scene["inter"], scene["vert_count"], scene["pred_scores"]
        gt_count = scene["gt_count"]
        preds = self.kept_proposals(scene, class_id)
        gts_all = np.flatnonzero(scene["gt_class"] == class_id)
        gts = gts_all[gt_count[gts_all] >= self.min_region_sizes]
        cur_true = np.ones(len(gts))
        cur_score = np.ones(len(gts)) * (-float("inf"))
        cur_match = np.zeros(len(gts), dtype=bool)
        visited = set()
        hard_false_negatives = 0
        for gti, g in enumerate(gts):       # greedy, in proposal order
            found_match = False
            for p in preds:
                if inter[p, g] <= 0 or p in visited:
                    continue
                overlap = float(inter[p, g]) / (gt_count[g] + vert[p] - inter[p, g])
                if overlap <= overlap_th:
                    continue
                if cur_match[gti]:   # a second proposal on a matched instance: the lower score is a false positive
                    low, high = min(cur_score[gti], score[p]), max(cur_score[gti], score[p])
                    cur_score[gti] = high
                    cur_true = np.append(cur_true, 0)
                    cur_score = np.append(cur_score, low)
                    cur_match = np.append(cur_match, True)
                else:
                    found_match = True
                    cur_match[gti] = True
                    cur_score[gti] = score[p]
                    visited.add(p)
            if not found_match:
                hard_false_negatives += 1
        cur_true, cur_score = cur_true[cur_match], cur_score[cur_match]
        for p in preds:                     # proposals that reach no instance of their class: false positives, unless
            row = inter[p, gts_all]         # they lie mostly on void points and on instances too small to count
            hit = row > 0
            row, count = row[hit], gt_count[gts_all][hit]
            if np.any(row.astype(np.float64) / (count + vert[p] - row) > overlap_th):
                continue
            num_ignore = scene["void_intersection"][p] + row[count < self.min_region_sizes].sum()
            if float(num_ignore) / vert[p] <= overlap_th:
                cur_true = np.append(cur_true, 0)
                cur_score = np.append(cur_score, score[p])
        return cur_true, cur_score, hard_false_negatives, len(gts) > 0, len(preds) > 0

    def evaluate_matches(self, scenes):
        if self.valid_class_ids is None:
            self.before_train()
        overlaps = self.overlaps
        ap_table = np.zeros((1, len(self.valid_class_ids), len(overlaps)), float)
        for oi, overlap_th in enumerate(overlaps):
            for li, class_id in enumerate(self.valid_class_ids):
                y_true, y_score = np.empty(0), np.empty(0)
                hard_false_negatives, has_gt, has_pred = 0, False, False
                for scene in scenes:
                    cur_true, cur_score, hard, any_gt, any_pred = self._match_scene(scene, class_id, overlap_th)
                    y_true, y_score = np.append(y_true, cur_true), np.append(y_score, cur_score)
                    hard_false_negatives += hard
                    has_gt, has_pred = has_gt or any_gt, has_pred or any_pred
                if has_gt and has_pred:
                    ap_current = average_precision(y_true, y_score, hard_false_negatives)
                elif has_gt:
                    ap_current = 0.0
                else:
                    ap_current = float("nan")
                ap_table[0, li, oi] = ap_current
        d_inf = 0
        o50 = np.where(np.isclose(self.overlaps, 0.5))
        o25 = np.where(np.isclose(self.overlaps, 0.25))
        o_all_but25 = np.where(np.logical_not(np.isclose(self.overlaps, 0.25)))
        ap_scores = dict()
        ap_scores["all_ap"] = np.nanmean(ap_table[d_inf, :, o_all_but25])
        ap_scores["all_ap_50%"] = np.nanmean(ap_table[d_inf, :, o50])
        ap_scores["all_ap_25%"] = np.nanmean(ap_table[d_inf, :, o25])
        ap_scores["classes"] = {}
        for li, label_name in enumerate(self.valid_class_names):
            ap_scores["classes"][label_name] = {
                "ap": np.average(ap_table[d_inf, li, o_all_but25]),
                "ap50%": np.average(ap_table[d_inf, li, o50]),
                "ap25%": np.average(ap_table[d_inf, li, o25]),
            }
        return ap_scores

    def _device_results_owner(self):
        model = self.trainer.model
        for m in (model, getattr(model, "module", None)):
            if hasattr(m, "set_device_results"):
                return m
        return None

    def eval(self):
        trainer = self.trainer
        trainer.logger.info(">>>>>>>>>>>>>>>> Start Evaluation >>>>>>>>>>>>>>>>")
        trainer.model.eval()
        owner = self._device_results_owner()
        previous = getattr(owner, "_device_results", False)
        if owner is not None:
            owner.set_device_results(True)
        scenes, losses = {}, []
        try:
            for input_dict in trainer.val_loader:
                assert len(input_dict["offset"]) == 1   # currently only support bs 1 for each GPU
                data_name = input_dict.pop("name")[0]
                _to_device(input_dict)
                with torch.no_grad():
                    output_dict = trainer.model(input_dict)
                segment, instance, idx = input_dict["segment"], input_dict["instance"], None
                if "origin_coord" in input_dict.keys():   # map to origin
                    idx, _ = pointops.knn_query(1, input_dict["coord"].float(), input_dict["offset"].int(),
                                                input_dict["origin_coord"].float(), input_dict["origin_offset"].int())
                    idx = idx.flatten()
                    segment, instance = input_dict["origin_segment"], input_dict["origin_instance"]
                scenes[data_name] = self.associate_instances(output_dict, segment, instance, idx)
                losses.append(output_dict["loss"])
        finally:
            if owner is not None:
                owner.set_device_results(previous)
        _, losses = _read_epoch(None, losses)
        for i, loss in enumerate(losses):
            trainer.logger.info("Test: [{iter}/{max_iter}] Loss {loss:.4f} ".format(iter=i + 1, max_iter=len(losses),
                                                                                   loss=loss))
        loss_avg = _mean(losses)
        comm.synchronize()
        scenes_sync = comm.gather(scenes, dst=0)

        if comm.is_main_process():
            scenes = {}
            for _ in range(len(scenes_sync)):
                scenes.update(scenes_sync.pop())
            self.scenes = scenes                     # name -> compact tables of this evaluation
            ap_scores = self.evaluate_matches(list(scenes.values()))
            self.ap_scores = ap_scores
            all_ap = ap_scores["all_ap"]
            all_ap_50 = ap_scores["all_ap_50%"]
            all_ap_25 = ap_scores["all_ap_25%"]
            trainer.logger.info("Val result: mAP/AP50/AP25 {:.4f}/{:.4f}/{:.4f}.".format(all_ap, all_ap_50, all_ap_25))
            for i, label_name in enumerate(self.valid_class_names):
                ap = ap_scores["classes"][label_name]
                trainer.logger.info("Class_{idx}-{name} Result: AP/AP50/AP25 {AP:.4f}/{AP50:.4f}/{AP25:.4f}".format(
                    idx=i, name=label_name, AP=ap["ap"], AP50=ap["ap50%"], AP25=ap["ap25%"]))
            current_epoch = trainer.epoch + 1
            if trainer.writer is not None:
                scalars = {"val/loss": loss_avg, "val/mAP": all_ap, "val/AP50": all_ap_50, "val/AP25": all_ap_25}
                for key, value in scalars.items():
                    trainer.writer.add_scalar(key, value, current_epoch)
                if trainer.cfg.enable_wandb:
                    wandb = _wandb()
                    wandb.log({"Epoch": current_epoch, **scalars}, step=wandb.run.step)
            trainer.logger.info("<<<<<<<<<<<<<<<<< End Evaluation <<<<<<<<<<<<<<<<<")
            trainer.comm_info["current_metric_value"] = all_ap_50   # save for saver
            trainer.comm_info["current_metric_name"] = "AP50"       # save for saver

    def after_train(self):
        self.trainer.logger.info("Best {}: {:.4f}".format("AP50", self.trainer.best_metric_value))
