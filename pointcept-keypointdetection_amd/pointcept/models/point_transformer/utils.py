"""LayerNorm1d of the reference's pointcept/models/point_transformer/utils.py:7-14: despite its name a BatchNorm1d over
the LAST axis of an (n, nsample, c) tensor (same parameters, buffers and state_dict keys as nn.BatchNorm1d)."""
import torch.nn as nn


class LayerNorm1d(nn.BatchNorm1d):
    def forward(self, x):
        # every (point, neighbour) pair is one row of the batch: statistics per channel over all the leading axes
        return super().forward(x.reshape(-1, x.shape[-1])).view(x.shape)
