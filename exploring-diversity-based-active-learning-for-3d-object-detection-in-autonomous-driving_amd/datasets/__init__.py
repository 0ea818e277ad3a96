from .anchors import AnchorGeneratorRange, create_anchors_3d_range, generate_task_anchors
from .target_assigner import NearestIouSimilarity, TargetAssigner
from .pool import PoolFrames, DeviceSweepLoader, CameraLidarSweepLoader
from .file_loader import FileSweepLoader, SweepFileReader
from .camera_files import CameraLidarFileLoader, ImageAugTest
from .pipelines import (PIPELINES, Compose, LoadPointCloudFromFile, LoadPointCloudAnnotations, Preprocess,
                        Voxelization, AssignTarget, Reformat, SweepDataset, collate_device)
from .create_gt_database import create_groundtruth_database, SweepPointsLoader, GtDatabaseWriter
from .db_sampler import (BatchSampler, DBFilterByDifficulty, DBFilterByMinNumPoint, DataBasePreprocessor, DataBaseSamplerV2,
                         build_dbsampler)
from .augment import augment_batch, TrainAugmenter

__all__ = ["BatchSampler", "DBFilterByDifficulty", "DBFilterByMinNumPoint", "DataBasePreprocessor", "DataBaseSamplerV2",
           "build_dbsampler", "augment_batch", "TrainAugmenter", "AnchorGeneratorRange", "NearestIouSimilarity", "TargetAssigner", "create_groundtruth_database", "SweepPointsLoader", "GtDatabaseWriter", "create_anchors_3d_range", "generate_task_anchors", "PoolFrames", "DeviceSweepLoader", "CameraLidarSweepLoader", "FileSweepLoader", "SweepFileReader", "CameraLidarFileLoader", "ImageAugTest", "PIPELINES",
           "Compose", "LoadPointCloudFromFile", "LoadPointCloudAnnotations", "Preprocess", "Voxelization",
           "AssignTarget", "Reformat", "SweepDataset", "collate_device"]
