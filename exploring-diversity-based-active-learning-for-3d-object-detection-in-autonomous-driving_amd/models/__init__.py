from .registry import (BACKBONES, DETECTORS, ESTIMATORS, HEADS, LOSSES, NECKS, READERS,
                       ROI_EXTRACTORS, SHARED_HEADS)
from .builder import build_backbone, build_detector, build_estimator, build_head, build_neck, build_reader
from .readers import (DynamicPillarFeatureNet, PillarFeatureNet, SimpleVoxel, VFELayer, VFEV3_ablation,
                      VoxelFeatureExtractor, VoxelFeatureExtractorV2, VoxelFeatureExtractorV3)
from .backbones import FPNSpMiddleResNetFHD, PointPillarsScatter, SparseTensor, SpMiddleFHD, SpMiddleResNetFHD
from .necks import RPN
from .bbox_heads import Head, MultiGroupHead
from .detectors import FPNVoxelNet, PointPillars, VoxelNet
from .box_coder import GroundBox3dCoderTorch, build_box_coder
from .bevfusion_camera import ConvFuser, DepthLSSTransform, GeneralizedLSSFPN, LSSViewTransform
from .transfusion_head import TransFusionHead
from .center_head import CenterHead, SeparateHead
from .swin import SwinTransformer
from .bevfusion_model import BEVFusion, BEVFusionCameraLidar
from .bevfusion_camera_only import BEVFusionCameraOnly, GeneralizedResNet, LSSFPN, LSSTransform
from .bev_seg_head import BEVGridTransform, BEVSegmentationHead
from .voxel_layers import DynamicScatter, Voxelization, dynamic_scatter
from .estimator import Estimator, WithEstimator

__all__ = ["READERS", "BACKBONES", "NECKS", "HEADS", "DETECTORS", "ESTIMATORS", "build_detector", "build_estimator",
           "build_reader", "build_backbone", "build_neck", "build_head", "build_box_coder"]
