"""Seeded parameters of the KeypointPTv3Plus fixture, shared by make_golden_keypoint_ptv3_plus.py and the tests.

The tiny Plus model has 0.65 M parameters, half of them in the ten 5^3 convolutions: stored as numbers they would take
2.6 MB.  They are random anyway, so the fixture stores the recipe instead: every entry of the state dict is drawn from
numpy's RandomState (the legacy MT19937 generator, whose streams numpy keeps frozen across versions) seeded by the
entry's own name, so the maker (which loads them into the reference class, strict) and the tests (which load them into
this package's class, strict) get the same bits from the key / shape listing of their own model.
LayerNorm / BatchNorm weights and every bias are drawn away from their initial 1 / 0 so that no affine term is trivial.
"""
import zlib

import numpy as np
import torch

SEED = 20260


def seeded_state_dict(template, seed=SEED):
    """template: a state_dict (names, shapes and dtypes are read, values ignored) -> dict of fresh CPU tensors."""
    out = {}
    for name, ref in template.items():
        rs = np.random.RandomState((seed + zlib.crc32(name.encode())) % (2 ** 32))
        shape = tuple(ref.shape)
        if name.endswith("num_batches_tracked"):
            v = np.zeros(shape, dtype=np.int64)
        elif name.endswith("running_var"):
            v = rs.uniform(0.5, 1.5, shape)
        elif name.endswith("running_mean"):
            v = 0.1 * rs.standard_normal(shape)
        elif len(shape) >= 2:                    # Linear (out, in) / sparse conv (out, k, k, k, in)
            v = rs.standard_normal(shape) / np.sqrt(np.prod(shape[1:]))
        elif name.endswith("weight"):            # LayerNorm / BatchNorm scale
            v = 1.0 + 0.1 * rs.standard_normal(shape)
        else:                                    # every bias
            v = 0.05 * rs.standard_normal(shape)
        out[name] = torch.from_numpy(np.asarray(v)).to(ref.dtype)
    return out
