"""KeypointEvaluator on the HIP path: same hook name, constructor, log line and comm_info as the reference
(pointcept/engines/hooks/keypoint_evaluator.py:10-84).  The reference reads two numbers back per batch (`.item()`)
and all-reduces them separately; here the totals stay on the device, and an epoch ends with one all-reduce and one
host read."""
import torch
import torch.distributed as dist

import pointcept.utils.comm as comm
from pointcept.engines.hooks.builder import HOOKS
from pointcept.engines.hooks import HookBase


def evaluate_batch(pred, target, scale=None):
    """Device vector [sum over samples of mean_k ||pred - target||_2 * scale, #samples] of one batch (:37-58)."""
    if target.shape != pred.shape:
        target = target.view(pred.shape)
    dist_val = torch.norm(pred.float() - target.float(), p=2, dim=-1).mean(dim=1)   # (B,)
    if scale is not None:
        dist_val = dist_val * scale.float().view(-1)
    return torch.stack([dist_val.sum(), dist_val.new_tensor(float(dist_val.shape[0]))])


@HOOKS.register_module()
class KeypointEvaluator(HookBase):
    def __init__(self):
        pass

    def after_epoch(self):
        if self.trainer.val_loader is not None:
            self.eval()

    def eval(self):
        self.trainer.model.eval()
        self.trainer.logger.info(">>>>>>>>>>>>>>>> Start Evaluation >>>>>>>>>>>>>>>>")
        totals = None
        with torch.no_grad():
            for data_dict in self.trainer.val_loader:
                for key in data_dict.keys():
                    if isinstance(data_dict[key], torch.Tensor):
                        data_dict[key] = data_dict[key].cuda(non_blocking=True)
                pred = self.trainer.model(data_dict)["pred"]
                t = evaluate_batch(pred, data_dict["target"], data_dict.get("scale", None))
                totals = t if totals is None else totals + t
        if totals is None:
            totals = torch.zeros(2, device="cuda")
        if comm.get_world_size() > 1:
            dist.all_reduce(totals)
        total_dist, total_samples = totals.tolist()   # the one host read of the evaluation
        mean_dist = total_dist / (total_samples + 1e-6)
        self.trainer.logger.info(f"Eval Result: Mean Distance = {mean_dist:.4f}")
        # negative: CheckpointSaver keeps the larger value (reference :79-84)
        self.trainer.comm_info["current_metric_value"] = -mean_dist
        self.trainer.comm_info["current_metric_name"] = "mean_dist"
