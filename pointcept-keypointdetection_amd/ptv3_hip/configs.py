"""Model configurations of the path as plain dicts (data only): the fork's keypoint-offset config and the small
plumbing configs the tests / smoke run use.  Keys are the constructor keywords of "PT-v3m1" / "PT-v3m2"."""
ORDERS = ["z", "z-trans", "hilbert", "hilbert-trans"]

# plumbing-size "PT-v3m1"
TINY_CFG = dict(
    in_channels=4, order=ORDERS, stride=(2, 2, 2, 2),
    enc_depths=(1, 1, 1, 2, 1), enc_channels=(16, 16, 32, 32, 64), enc_num_head=(1, 1, 2, 2, 4),
    enc_patch_size=(64,) * 5, dec_depths=(1, 1, 1, 1), dec_channels=(16, 16, 32, 32),
    dec_num_head=(1, 1, 2, 2), dec_patch_size=(64,) * 4, mlp_ratio=4, qkv_bias=True,
    drop_path=0.3, shuffle_orders=True, pre_norm=True, enable_rpe=False, enable_flash=False,
    upcast_attention=False, upcast_softmax=False,
)

# the fork's config (configs/my_dataset/offset_keypoint_ptv3.py:11-46)
FORK_CFG = dict(
    in_channels=4, order=ORDERS, stride=(2, 2, 2, 2),
    enc_depths=(2, 2, 2, 6, 2), enc_channels=(32, 64, 128, 256, 512), enc_num_head=(2, 4, 8, 16, 32),
    enc_patch_size=(1024,) * 5, dec_depths=(2, 2, 2, 2), dec_channels=(64, 64, 128, 256),
    dec_num_head=(4, 4, 8, 16), dec_patch_size=(1024,) * 4, mlp_ratio=4, qkv_bias=True, qk_scale=None,
    attn_drop=0.0, proj_drop=0.0, drop_path=0.3, shuffle_orders=True, pre_norm=True, enable_rpe=False,
    enable_flash=False, upcast_attention=False, upcast_softmax=False,
)

# the upstream PTv3 semantic-segmentation backbone (configs/scannet/semseg-pt-v3m1-0-base.py:14-44,
# configs/nuscenes/semseg-pt-v3m1-0-base.py): same widths as the fork, enable_flash=True, 1024-point patches
SEMSEG_CFG = dict(FORK_CFG, enable_flash=True)

# the fork's segmentation criteria (configs/pigseg/semseg-{ptv3,swin3d,octformer}-v1m1-0-base.py share this list) and
# the `model` dict of configs/pigseg/semseg-ptv3-v1m1-0-base.py:34-70
PIGSEG_CRITERIA = [
    dict(type="FocalLoss", gamma=2.0, alpha=[0.1, 0.9], loss_weight=1.0, ignore_index=-1),
    dict(type="LovaszLoss", mode="multiclass", loss_weight=3.0, ignore_index=-1),
]
PIGSEG_PTV3_CFG = dict(type="DefaultSegmentorV2", num_classes=2, backbone_out_channels=64,
                       backbone=dict(type="PT-v3m1", **FORK_CFG), criteria=PIGSEG_CRITERIA)

# the fork's body-size-and-weight regression: the `model` dict of configs/my_dataset/ptv3_weight.py:40-77, verbatim (no
# dec_* keys: the backbone's defaults hold; enc_num_head gives head dimension 32 at every encoder level)
PIG_WEIGHT_PTV3_CFG = dict(
    type="PigBodyRegressor",
    criteria=[dict(type="RegressionL1Loss", loss_weight=1.0)],
    num_classes=7,
    backbone_embed_dim=64,
    backbone=dict(
        type="PT-v3m1",
        in_channels=4,
        order=("z", "z-trans", "hilbert", "hilbert-trans"),
        stride=(2, 2, 2, 2),
        enc_depths=(2, 2, 2, 6, 2),
        enc_channels=(32, 64, 128, 256, 512),
        enc_num_head=(1, 2, 4, 8, 16),
        enc_patch_size=(1024, 1024, 1024, 1024, 1024),
        dec_patch_size=(1024, 1024, 1024, 1024),
        mlp_ratio=4,
        qkv_bias=True,
        qk_scale=None,
        attn_drop=0.0,
        proj_drop=0.0,
        drop_path=0.3,
        shuffle_orders=True,
        pre_norm=True,
        enable_rpe=False,
        enable_flash=False,
        upcast_attention=False,
        upcast_softmax=False,
        pdnorm_bn=False,
        pdnorm_ln=False,
        pdnorm_decouple=True,
        pdnorm_adaptive=False,
        pdnorm_affine=True,
        pdnorm_conditions=("nuisance", 3),
    ),
)

# "PT-v3m2" (point_transformer_v3m2_sonata.py) plumbing-size config: GridPooling, LayerScale, LayerNorm stem
TINY_M2_CFG = dict(
    in_channels=4, order=ORDERS, stride=(2, 2, 2, 2),
    enc_depths=(1, 1, 1, 2, 1), enc_channels=(16, 16, 32, 32, 64), enc_num_head=(1, 1, 2, 2, 4),
    enc_patch_size=(64,) * 5, dec_depths=(1, 1, 1, 1), dec_channels=(16, 16, 32, 32),
    dec_num_head=(1, 1, 2, 2), dec_patch_size=(64,) * 4, mlp_ratio=4, qkv_bias=True,
    drop_path=0.3, layer_scale=0.5, shuffle_orders=True, pre_norm=True, enable_rpe=False, enable_flash=False,
    upcast_attention=False, upcast_softmax=False,
)

# Swin3D-S backbone of configs/s3dis/semseg-swin3d-v1m1-0-small.py:11-30 (built there under "DefaultSegmentor")
SWIN3D_S3DIS_CFG = dict(
    type="Swin3D-v1m1", in_channels=9, num_classes=13, base_grid_size=0.02, depths=[2, 4, 9, 4, 4],
    channels=[48, 96, 192, 384, 384], num_heads=[6, 6, 12, 24, 24], window_sizes=[5, 7, 7, 7, 7], quant_size=4,
    drop_path_rate=0.3, up_k=3, num_layers=5, stem_transformer=True, down_stride=3, upsample="linear_attn",
    knn_down=True, cRSE="XYZ_RGB_NORM", fp16_mode=1,
)

# the fork's Swin3D offset model (configs/my_dataset/offset_keypoint_swin3d.py:11-40)
OFFSET_SWIN3D_CFG = dict(
    type="OffsetKeypointSwin3D", num_keypoints=6, hidden_dim=256,
    backbone_conf=dict(
        type="Swin3D-v1m1", in_channels=4, num_classes=64, base_grid_size=0.02, quant_size=50, num_layers=4,
        depths=[2, 2, 6, 2], channels=[64, 128, 256, 512], num_heads=[4, 8, 16, 32], window_sizes=[5, 7, 7, 7],
        up_k=3, drop_path_rate=0.2, stem_transformer=True, down_stride=2, upsample="linear", knn_down=True,
        cRSE="XYZ_RGB", fp16_mode=1,
    ),
)

# the fork's global-regression models (configs/my_dataset/keypoint_ptv3.py:11-47, keypoint_swin3d.py:11-42)
KEYPOINT_PTV3_CFG = dict(
    type="KeypointPTv3", num_keypoints=6,
    backbone_conf=dict(type="PT-v3m1", **FORK_CFG, pdnorm_bn=False, pdnorm_ln=False, pdnorm_decouple=True,
                       pdnorm_adaptive=False, pdnorm_affine=True,
                       pdnorm_conditions=("ScanNet", "S3DIS", "Structured3D")),
)
# the fork's own backbone (configs/my_dataset/keypoint_ptv3_plus.py:11-56): PT-v3m1 widths, bottleneck 5^3 xCPE
KEYPOINT_PTV3_PLUS_CFG = dict(
    type="KeypointPTv3Plus", num_keypoints=6, hidden_dim=256,
    backbone_conf=dict(KEYPOINT_PTV3_CFG["backbone_conf"], type="PT-v3m1-Plus", cpe_kernel_size=5),
)
KEYPOINT_SWIN3D_CFG = dict(OFFSET_SWIN3D_CFG, type="KeypointSwin3D",
                           backbone_conf=dict(OFFSET_SWIN3D_CFG["backbone_conf"]))
# the fork's voting model (configs/my_dataset/keypoint_swin3d_plus.py:14-52)
KEYPOINT_SWIN3D_VOTE_CFG = dict(OFFSET_SWIN3D_CFG, type="KeypointSwin3DVote", vote_radius=0.3,
                                backbone_conf=dict(OFFSET_SWIN3D_CFG["backbone_conf"]))
# the fork's Point Transformer V1 regression model (configs/my_dataset/keypoint_ptv1.py:20-28)
KEYPOINT_PTV1_CFG = dict(type="KeypointPTv1-50", in_channels=7, num_keypoints=6, hidden_dim=256)
# the fork's OA-CNNs regression model (configs/my_dataset/keypoint_oa_cnns.py:12-29), run at batch size 8
KEYPOINT_OACNNS_CFG = dict(
    type="KeypointOACNNs", num_keypoints=6, in_channels=4, embed_channels=64, enc_channels=[64, 64, 128, 256],
    groups=[4, 4, 8, 16], enc_depth=[3, 3, 9, 8], dec_channels=[256, 256, 256, 256],
    point_grid_size=[[8, 12, 16, 16], [6, 9, 12, 12], [4, 6, 8, 8], [3, 4, 6, 6]], dec_depth=[2, 2, 2, 2],
    enc_num_ref=[16, 16, 16, 16], hidden_dim=256,
)
# the fork's SpUNet regression model (configs/my_dataset/keypoint_sparse_unet.py:16-34), run at batch size 8
KEYPOINT_SPUNET_CFG = dict(
    type="KeypointSparseUNet", num_keypoints=6, in_channels=4, num_classes=0, base_channels=32,
    channels=(32, 64, 128, 256, 256, 128, 96, 96), layers=(2, 3, 4, 6, 2, 2, 2, 2), enc_mode=False, hidden_dim=256,
)

# the fork's Point Transformer V2 regression model (configs/my_dataset/keypoint_ptv2.py:11-54), run at batch size 8
KEYPOINT_PTV2_CFG = dict(
    type="KeypointPTv2", num_keypoints=6, hidden_dim=256,
    backbone_conf=dict(
        type="PT-v2m2", in_channels=4, num_classes=0, patch_embed_depth=1, patch_embed_channels=48,
        patch_embed_groups=6, patch_embed_neighbours=8, enc_depths=(2, 2, 6, 2), enc_channels=(96, 192, 384, 512),
        enc_groups=(12, 24, 48, 64), enc_neighbours=(16, 16, 16, 16), dec_depths=(1, 1, 1, 1),
        dec_channels=(48, 96, 192, 384), dec_groups=(6, 12, 24, 48), dec_neighbours=(16, 16, 16, 16),
        grid_sizes=(0.06, 0.12, 0.24, 0.48), attn_qkv_bias=True, pe_multiplier=False, pe_bias=True, attn_drop_rate=0.0,
        drop_path_rate=0.3, enable_checkpoint=False, unpool_backend="map"),
)

# the fork's Stratified Transformer regression model (configs/my_dataset/keypoint_stratified_transformer.py:12-45), run at
# batch size 8
KEYPOINT_STRAT_CFG = dict(
    type="KeypointStratifiedTransformer", num_keypoints=6, in_channels=4, channels=[48, 96, 192, 384, 384],
    num_heads=[6, 12, 24, 24], depths=[3, 9, 3, 3], window_size=[0.2, 0.4, 0.8, 1.6],
    quant_size=[0.01, 0.02, 0.04, 0.08], mlp_expend_ratio=4.0, down_ratio=0.25, down_num_sample=16, kp_ball_radius=0.05,
    kp_max_neighbor=34, kp_grid_size=0.02, kp_sigma=1.0, drop_path_rate=0.2, rel_query=True, rel_key=True,
    rel_value=True, qkv_bias=True, stem=True, hidden_dim=256,
)

# the fork's OctFormer regression and per-point offset models (configs/my_dataset/keypoint_octformer.py:15-35 and
# offset_keypoint_octformer.py:14-32), run at batch size 8
KEYPOINT_OCTFORMER_CFG = dict(
    type="KeypointOctFormer", in_channels=4, num_keypoints=6, fpn_channels=168, hidden_dim=256,
    channels=(96, 192, 384, 384), num_blocks=(2, 2, 18, 2), num_heads=(6, 12, 24, 24), patch_size=26, stem_down=2,
    head_up=2, dilation=4, drop_path=0.5, nempty=True, octree_depth=11, octree_full_depth=2, octree_scale_factor=10.24,
)
OFFSET_KEYPOINT_OCTFORMER_CFG = dict(KEYPOINT_OCTFORMER_CFG, type="OffsetKeypointOctFormer")

# plumbing-size Swin3D: three levels, both head widths the kernel is built for (8 and 16)
TINY_SWIN3D_CFG = dict(
    type="Swin3D-v1m1", in_channels=9, num_classes=13, base_grid_size=0.02, depths=[2, 2, 2], channels=[16, 32, 32],
    num_heads=[2, 2, 2], window_sizes=[5, 7, 7], quant_size=4, drop_path_rate=0.3, up_k=3, num_layers=3,
    stem_transformer=True, down_stride=3, upsample="linear_attn", knn_down=True, cRSE="XYZ_RGB_NORM", fp16_mode=1,
)

# the two constructor variants no shipped config uses: GridDownsample (knn_down=False) and the residual stem
# (stem_transformer=False) - tests/golden/state_dict_swin3d_tiny_grid_resstem.txt lists the reference class built this way
TINY_SWIN3D_GRID_RESSTEM_CFG = dict(TINY_SWIN3D_CFG, knn_down=False, stem_transformer=False)

# PointGroup instance segmentation on ScanNet: the `model` dicts of configs/scannet/insseg-pointgroup-v1m2-0-ptv3-base.py
# :37-90 (PG-v1m2 on the PT-v3m1 of bench.py) and configs/scannet/insseg-pointgroup-v1m1-0-spunet-base.py:37-55
_PG_SCANNET = dict(semantic_num_classes=20, semantic_ignore_index=-1, segment_ignore_index=(-1, 0, 1),
                   instance_ignore_index=-1, cluster_thresh=1.5, cluster_closed_points=300, cluster_propose_points=100,
                   cluster_min_points=50)
PG_PTV3_SCANNET_CFG = dict(
    type="PG-v1m2",
    backbone=dict(
        type="PT-v3m1", in_channels=6, order=("z", "z-trans", "hilbert", "hilbert-trans"), stride=(2, 2, 2, 2),
        enc_depths=(2, 2, 2, 6, 2), enc_channels=(32, 64, 128, 256, 512), enc_num_head=(2, 4, 8, 16, 32),
        enc_patch_size=(1024, 1024, 1024, 1024, 1024), dec_depths=(2, 2, 2, 2), dec_channels=(64, 64, 128, 256),
        dec_num_head=(4, 4, 8, 16), dec_patch_size=(1024, 1024, 1024, 1024), mlp_ratio=4, qkv_bias=True, qk_scale=None,
        attn_drop=0.0, proj_drop=0.0, drop_path=0.3, shuffle_orders=True, pre_norm=True, enable_rpe=False,
        enable_flash=True, upcast_attention=False, upcast_softmax=False, enc_mode=False, pdnorm_bn=False,
        pdnorm_ln=False, pdnorm_decouple=True, pdnorm_adaptive=False, pdnorm_affine=True,
        pdnorm_conditions=("ScanNet", "S3DIS", "Structured3D")),
    backbone_out_channels=64, **_PG_SCANNET,
    criteria=[dict(type="CrossEntropyLoss", loss_weight=1.0, ignore_index=-1),
              dict(type="LovaszLoss", mode="multiclass", loss_weight=1.0, ignore_index=-1)],
)
PG_SPUNET_SCANNET_CFG = dict(
    type="PG-v1m1",
    backbone=dict(type="SpUNet-v1m1", in_channels=6, num_classes=0, channels=(32, 64, 128, 256, 256, 128, 96, 96),
                  layers=(2, 3, 4, 6, 2, 2, 2, 2)),
    backbone_out_channels=96, **_PG_SCANNET,
)

# Context-aware classifier: the `model` dicts of configs/scannet/semseg-cac-v1m1-1-spunet-lovasz.py:10-33 and
# configs/scannet200/semseg-cac-v1m1-2-ptv2-lovasz.py:14-57
_CAC_CRITERIA = [dict(type="CrossEntropyLoss", loss_weight=1.0, ignore_index=-1),
                 dict(type="LovaszLoss", mode="multiclass", loss_weight=1.0, ignore_index=-1)]
CAC_SPUNET_SCANNET_CFG = dict(
    type="CAC-v1m1",
    backbone=dict(type="SpUNet-v1m1", in_channels=6, num_classes=0, channels=(32, 64, 128, 256, 256, 128, 96, 96),
                  layers=(2, 3, 4, 6, 2, 2, 2, 2)),
    criteria=_CAC_CRITERIA, num_classes=20, backbone_out_channels=96, cos_temp=15, main_weight=1, pre_weight=1,
    pre_self_weight=1, kl_weight=1, conf_thresh=0.75, detach_pre_logits=True,
)
CAC_PTV2_SCANNET200_CFG = dict(
    type="CAC-v1m1",
    backbone=dict(
        type="PT-v2m2", in_channels=9, num_classes=0, patch_embed_depth=1, patch_embed_channels=48,
        patch_embed_groups=6, patch_embed_neighbours=8, enc_depths=(2, 2, 6, 2), enc_channels=(96, 192, 384, 512),
        enc_groups=(12, 24, 48, 64), enc_neighbours=(16, 16, 16, 16), dec_depths=(1, 1, 1, 1),
        dec_channels=(48, 96, 192, 384), dec_groups=(6, 12, 24, 48), dec_neighbours=(16, 16, 16, 16),
        grid_sizes=(0.06, 0.15, 0.375, 0.9375), attn_qkv_bias=True, pe_multiplier=False, pe_bias=True,
        attn_drop_rate=0.0, drop_path_rate=0.3, enable_checkpoint=False, unpool_backend="map"),
    criteria=_CAC_CRITERIA, num_classes=200, backbone_out_channels=48, cos_temp=15, main_weight=1, pre_weight=1,
    pre_self_weight=1, kl_weight=1, conf_thresh=0, detach_pre_logits=True,
)

# Point Prompt Training: the `model` dict of configs/scannet/semseg-pt-v3m1-1-ppt-extreme.py:30-92 (class_name and
# valid_index are the class defaults there and here), and a tiny PPT-v1m2 (decoupled heads) on PT-v3m1
PPT_PTV3_SCANNET_CFG = dict(
    type="PPT-v1m1",
    backbone=dict(
        type="PT-v3m1", in_channels=6, order=("z", "z-trans", "hilbert", "hilbert-trans"), stride=(2, 2, 2, 2),
        enc_depths=(3, 3, 3, 6, 3), enc_channels=(48, 96, 192, 384, 512), enc_num_head=(3, 6, 12, 24, 32),
        enc_patch_size=(1024, 1024, 1024, 1024, 1024), dec_depths=(3, 3, 3, 3), dec_channels=(64, 96, 192, 384),
        dec_num_head=(4, 6, 12, 24), dec_patch_size=(1024, 1024, 1024, 1024), mlp_ratio=4, qkv_bias=True,
        qk_scale=None, attn_drop=0.0, proj_drop=0.0, drop_path=0.3, shuffle_orders=True, pre_norm=True,
        enable_rpe=False, enable_flash=True, upcast_attention=False, upcast_softmax=False, enc_mode=False,
        pdnorm_bn=True, pdnorm_ln=True, pdnorm_decouple=True, pdnorm_adaptive=False, pdnorm_affine=True,
        pdnorm_conditions=("ScanNet", "S3DIS", "Structured3D")),
    criteria=_CAC_CRITERIA, backbone_out_channels=64, context_channels=256,
    conditions=("Structured3D", "ScanNet", "S3DIS"), template="[x]", clip_model="ViT-B/16", backbone_mode=False,
)
PPT_V1M2_TINY_CFG = dict(
    type="PPT-v1m2",
    backbone=dict(
        type="PT-v3m1", in_channels=4, order=("z", "z-trans"), stride=(2, 2), enc_depths=(1, 1, 1),
        enc_channels=(16, 32, 64), enc_num_head=(1, 2, 4), enc_patch_size=(16, 16, 16), dec_depths=(1, 1),
        dec_channels=(16, 32), dec_num_head=(1, 2), dec_patch_size=(16, 16), drop_path=0.0, enable_flash=False,
        pdnorm_bn=True, pdnorm_ln=True, pdnorm_conditions=("A", "B", "C")),
    criteria=[dict(type="CrossEntropyLoss", loss_weight=1.0, ignore_index=-1)], backbone_out_channels=16,
    context_channels=256, conditions=("A", "B", "C"), num_classes=(5, 7, 3), backbone_mode=False,
)

# Point Prompt Training over the sparse U-Net: the `model` dict of configs/scannet/semseg-ppt-v1m1-0-sc-st-spunet.py:17-55
# (class_name and valid_index are the class defaults there and here), and the tiny SpUNet-v1m3 of the fixture
# tests/golden/make_golden_spunet_pdnorm.py
PPT_SPUNET_SCANNET_CFG = dict(
    type="PPT-v1m1",
    backbone=dict(type="SpUNet-v1m3", in_channels=6, num_classes=0, base_channels=32, context_channels=256,
                  channels=(32, 64, 128, 256, 256, 128, 96, 96), layers=(2, 3, 4, 6, 2, 2, 2, 2), enc_mode=False,
                  conditions=("ScanNet", "S3DIS", "Structured3D"), zero_init=False, norm_decouple=True,
                  norm_adaptive=True, norm_affine=True),
    criteria=[dict(type="CrossEntropyLoss", loss_weight=1.0, ignore_index=-1)], backbone_out_channels=96,
    context_channels=256, conditions=("Structured3D", "ScanNet", "S3DIS"), template="[x]", clip_model="ViT-B/16",
    backbone_mode=False,
)
SPUNET_PDNORM_TINY_CFG = dict(
    type="SpUNet-v1m3", in_channels=4, num_classes=0, base_channels=16, context_channels=24,
    channels=(16, 32, 32, 64, 64, 32, 16, 16), layers=(1, 2, 1, 1, 1, 1, 2, 1), enc_mode=False,
    conditions=("A", "B", "C"), zero_init=False, norm_decouple=True, norm_adaptive=True, norm_affine=True,
)

# Sonata pretraining: the `model` dict of configs/sonata/pretrain-sonata-v1m1-0-base.py:21-79, and a tiny one (three
# stages, up-cast back to the input level, 100 prototypes; no order shuffle, drop path or jitter, so that the patch
# permutation is the only random draw of a step)
SONATA_BASE_CFG = dict(
    type="Sonata-v1m1",
    backbone=dict(
        type="PT-v3m2", in_channels=9, order=("z", "z-trans", "hilbert", "hilbert-trans"), stride=(2, 2, 2, 2),
        enc_depths=(3, 3, 3, 12, 3), enc_channels=(48, 96, 192, 384, 512), enc_num_head=(3, 6, 12, 24, 32),
        enc_patch_size=(1024, 1024, 1024, 1024, 1024), mlp_ratio=4, qkv_bias=True, qk_scale=None, attn_drop=0.0,
        proj_drop=0.0, drop_path=0.3, shuffle_orders=True, pre_norm=True, enable_rpe=False, enable_flash=True,
        upcast_attention=False, upcast_softmax=False, traceable=True, enc_mode=True, mask_token=True),
    teacher_custom=dict(attn_drop=0.0, proj_drop=0.0, drop_path=0.0),
    head_in_channels=1088, head_hidden_channels=4096, head_embed_channels=256, head_num_prototypes=4096,
    num_global_view=2, num_local_view=4, mask_size_start=0.1, mask_size_base=0.4, mask_size_warmup_ratio=0.05,
    mask_ratio_start=0.3, mask_ratio_base=0.7, mask_ratio_warmup_ratio=0.05, mask_jitter=0.01, teacher_temp_start=0.04,
    teacher_temp_base=0.07, teacher_temp_warmup_ratio=0.05, student_temp=0.1, mask_loss_weight=2 / 8,
    roll_mask_loss_weight=2 / 8, unmask_loss_weight=4 / 8, momentum_base=0.994, momentum_final=1, match_max_k=8,
    match_max_r=0.32, up_cast_level=2,
)
SONATA_TINY_CFG = dict(
    type="Sonata-v1m1",
    backbone=dict(
        type="PT-v3m2", in_channels=4, order=("z", "z-trans"), stride=(2, 2), enc_depths=(1, 1, 1),
        enc_channels=(16, 16, 32), enc_num_head=(1, 1, 2), enc_patch_size=(16, 16, 16), drop_path=0.0,
        shuffle_orders=False, enable_flash=False, traceable=True, enc_mode=True, mask_token=True),
    head_in_channels=64, head_hidden_channels=64, head_embed_channels=16, head_num_prototypes=100,
    num_global_view=2, num_local_view=2, mask_size_start=1.0, mask_ratio_start=0.5, mask_jitter=None,
    match_max_r=0.04, up_cast_level=2,
)

# Concerto pretraining: the `model` dict of configs/concerto/pretrain-concerto-v1m1-0-base.py (Sonata's base backbone and
# schedules; the image branch carries half of the loss), and a tiny one (four stages, the heads at level 2, the image
# branch at level 1, 6 x 6 patches of a 24-channel encoder)
CONCERTO_BASE_CFG = dict(
    {k: v for k, v in SONATA_BASE_CFG.items() if k not in ("type", "head_in_channels")},
    type="Concerto-v1m1", patch_h=518 // 14, patch_w=518 // 14, image_weight_name="dinov2_vitg14_reg",
    image_weight_path="facebook/dinov2-with-registers-giant", backbone_out_channels=1184, embedding_channels=64,
    student_pretrained=False, enc2d_upcast_level=3, head_in_channels=1088, enc2d_head_in_channels=1536,
    enc2d_head_hidden_channels=4096, enc2d_head_embed_channels=256, enc2d_head_num_prototypes=4096,
    mask_loss_weight=1 / 8, roll_mask_loss_weight=1 / 8, unmask_loss_weight=2 / 8, enc2d_loss_weight=4 / 8,
    enc2d_cos_shift=True, sonata_model_type="online",
)
CONCERTO_TINY_CFG = dict(
    type="Concerto-v1m1", image_weight_name="stub", image_weight_path=None,
    backbone=dict(
        type="PT-v3m2", in_channels=4, order=("z", "z-trans"), stride=(2, 2, 2), enc_depths=(1, 1, 1, 1),
        enc_channels=(16, 16, 32, 32), enc_num_head=(1, 1, 2, 2), enc_patch_size=(16, 16, 16, 16), drop_path=0.0,
        shuffle_orders=False, enable_flash=False, traceable=True, enc_mode=True, mask_token=True),
    head_in_channels=64, backbone_out_channels=80, embedding_channels=16, patch_w=6, patch_h=6,
    head_hidden_channels=64, head_embed_channels=16, head_num_prototypes=100, enc2d_head_in_channels=24,
    enc2d_head_hidden_channels=32, enc2d_head_embed_channels=16, enc2d_head_num_prototypes=20, num_global_view=2,
    num_local_view=2, mask_size_start=1.0, mask_ratio_start=0.5, mask_jitter=None, match_max_r=0.04,
    mask_loss_weight=1 / 8, roll_mask_loss_weight=1 / 8, unmask_loss_weight=2 / 8, enc2d_loss_weight=4 / 8,
    up_cast_level=1, enc2d_upcast_level=2, enc2d_cos_shift=True, sonata_model_type="online",
)
