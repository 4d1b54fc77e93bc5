"""Process-group helpers the hooks use (reference: pointcept/utils/comm.py:23-90): thin views of torch.distributed."""
import functools

import torch.distributed as dist


def _on():
    return dist.is_available() and dist.is_initialized()


def get_world_size() -> int:
    return dist.get_world_size() if _on() else 1


def get_rank() -> int:
    return dist.get_rank() if _on() else 0


def is_main_process() -> bool:
    return get_rank() == 0


def synchronize():
    if _on() and dist.get_world_size() > 1:
        dist.barrier()


@functools.lru_cache()
def _get_global_gloo_group():
    """All ranks on the gloo backend, made once: pickled objects travel through host memory (:91-100)."""
    if dist.get_backend() == "nccl":
        return dist.new_group(backend="gloo")
    return dist.group.WORLD


def gather(data, dst=0, group=None):
    """Any picklable object from every rank (:128-155): on `dst` the list of them in rank order, elsewhere an empty list;
    [data] at world size 1."""
    if get_world_size() == 1:
        return [data]
    if group is None:
        group = _get_global_gloo_group()
    world_size = dist.get_world_size(group=group)
    if world_size == 1:
        return [data]
    if dist.get_rank(group=group) == dst:
        output = [None for _ in range(world_size)]
        dist.gather_object(data, output, dst=dst, group=group)
        return output
    dist.gather_object(data, None, dst=dst, group=group)
    return []
