"""build_* helpers (reference det3d/models/builder.py:17-58)."""
from torch import nn

from ..utils import build_from_cfg
from .registry import BACKBONES, DETECTORS, ESTIMATORS, HEADS, NECKS, READERS


def build(cfg, registry, default_args=None):
    if isinstance(cfg, list):
        return nn.Sequential(*[build_from_cfg(c, registry, default_args) for c in cfg])
    return build_from_cfg(cfg, registry, default_args)


def build_reader(cfg):
    return build(cfg, READERS)


def build_backbone(cfg):
    return build(cfg, BACKBONES)


def build_neck(cfg):
    return build(cfg, NECKS)


def build_head(cfg):
    return build(cfg, HEADS)


def build_detector(cfg, train_cfg=None, test_cfg=None):
    return build(cfg, DETECTORS, dict(train_cfg=train_cfg, test_cfg=test_cfg))


def build_estimator(cfg):
    return build(cfg, ESTIMATORS)
