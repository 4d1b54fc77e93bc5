from .prompt_driven_normalization import PDNorm  # noqa: F401
from .point_prompt_training_v1m1_language_guided import PointPromptTraining  # noqa: F401
from .point_prompt_training_v1m2_decoupled import PointPromptTrainingDecoupled  # noqa: F401
