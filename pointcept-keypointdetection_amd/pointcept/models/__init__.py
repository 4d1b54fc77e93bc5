"""pointcept.models on MI355X: registers only what the PTv3 / Swin3D window-attention path implements.

The reference's pointcept/models/__init__.py:1-45 imports every backbone (spconv, MinkowskiEngine,
ocnn, torch_cluster, peft ...) and cannot be imported on a ROCm box; this package replaces it.
"""
from .builder import MODELS, MODULES, build_model  # noqa: F401
from .default import DefaultSegmentor, DefaultSegmentorV2, DefaultClassifier  # noqa: F401
from .modules import PointModule, PointSequential, PointModel  # noqa: F401
from .point_transformer_v3 import *  # noqa: F401,F403
from .offset_keypoint_ptv3 import OffsetKeypointPTv3  # noqa: F401
from .swin3d import Swin3DUNet  # noqa: F401
from .offset_keypoint_swin3d import OffsetKeypointSwin3D  # noqa: F401
from .keypoint_ptv3 import KeypointPTv3  # noqa: F401
from .keypoint_swin3d import KeypointSwin3D  # noqa: F401
from .keypoint_swin3d_vote import KeypointSwin3DVote  # noqa: F401
from .keypoint_ptv1 import KeypointPTv1  # noqa: F401
from .oacnns import OACNNs  # noqa: F401
from .keypoint_oa_cnns import KeypointOACNNs  # noqa: F401
from .point_transformer_v2 import PointTransformerV2  # noqa: F401
from .keypoint_ptv2 import KeypointPTv2  # noqa: F401
from .keypoint_ptv3_plus import BlockPlus, PointTransformerV3Plus, KeypointPTv3Plus  # noqa: F401
from .sparse_unet import SpUNetBase  # noqa: F401
from .sparse_unet import PDBatchNorm, SpUNetBasePDNorm  # noqa: F401
from .keypoint_sparse_unet import KeypointSparseUNet  # noqa: F401
from .stratified_transformer import StratifiedTransformer  # noqa: F401
from .keypoint_stratified_transformer import KeypointStratifiedTransformer  # noqa: F401
from .octformer import OctFormer  # noqa: F401
from .keypoint_octformer import KeypointOctFormer  # noqa: F401
from .offset_keypoint_octformer import OffsetKeypointOctFormer  # noqa: F401
from .pig_regressor import PigBodyRegressor  # noqa: F401
from .point_group import PointGroup, PointGroupV1m2  # noqa: F401
from .context_aware_classifier import CACSegmentor  # noqa: F401
from .point_prompt_training import PDNorm, PointPromptTraining, PointPromptTrainingDecoupled  # noqa: F401
from .sonata import OnlineCluster, Sonata  # noqa: F401
from .concerto import Concerto  # noqa: F401
