"""Stratified Transformer (ST-v1m2) on MI355X."""
from .stratified_transformer_v1m2_refine import StratifiedTransformer  # noqa: F401
