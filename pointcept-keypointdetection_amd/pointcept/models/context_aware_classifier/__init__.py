from .context_aware_classifier_v1m1_base import CACSegmentor  # noqa: F401
