"""GPU suite: AL3D_MATH=auto on a camera detector.  The registered ``BEVFusion`` camera+lidar detector of
tests/test_bevfusion_camera_lidar_gpu.py (Swin-T backbone, no head), seeded weights, two batches of two frames.  One Swin
block is rescaled by a power of two -- the v rows of ``qkv.weight`` and the v part of ``qkv.bias`` times 2^18,
``proj.weight`` times 2^-18 -- which is the same function in exact arithmetic but puts v and the attention output beyond
65504: the f16x3 token kernels leave their range on every frame, and the sweep's recovery re-runs the batches on the bf16x6
token kernels (csrc/tokens_bf16x6.hip)."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, BATCH = 4, 2


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.fixture(scope="module")
def rig():
    from al3d import synthetic
    from al3d.datasets import PoolFrames
    from al3d.models import build_detector
    from al3d.utils import Config
    cfg = Config.fromfile(os.path.join(ROOT, "examples", "active", "bevfusion_camera_lidar_spatial_temporal_feature.py"))
    model = build_detector(cfg.model, train_cfg=None, test_cfg=cfg.test_cfg)
    synthetic.seeded_init_(model.lidar, seed=0)
    for i, m in enumerate((model.camera_backbone, model.camera_neck, model.vtransform, model.fuser)):
        synthetic.seed_modules_(m, 60 + i)
    return dict(cfg=cfg, model=model.to(DEV).eval(), pool=PoolFrames.from_synthetic(N, DEV, num_base=2, seed=11))


def _sweep(rig, math_=None, **kw):
    from al3d import detector_ops as D, sweep as S
    from al3d.datasets import CameraLidarSweepLoader
    saved = D.MATH
    try:
        if math_ is not None:
            D.MATH = math_
        loader = CameraLidarSweepLoader(rig["pool"], rig["cfg"].voxel_generator, None, BATCH, device=DEV, num_image_base=2,
                                        seed=5)
        out = S.sweep_embeddings(rig["model"], loader, DEV, N, **kw)
        torch.cuda.synchronize()
        return out
    finally:
        D.MATH = saved


def test_auto_recovers_a_swin_block_that_leaves_the_f16x3_range(rig):
    from al3d import detector_ops as D, sweep as S
    from al3d.lib import Al3dError
    assert D.MATH == "f16x3"
    plain6 = _sweep(rig, math_="bf16x6")                       # the un-rescaled model, bf16x6 from the start
    assert bool(torch.isfinite(plain6).all()) and float(plain6.abs().max()) > 0
    msa = rig["model"].camera_backbone.stages[2].blocks[1].attn.w_msa
    C = msa.embed_dims
    with torch.no_grad():                                      # in place: the packed-weight caches follow the versions
        msa.qkv.weight[2 * C:].mul_(2.0 ** 18)
        msa.qkv.bias[2 * C:].mul_(2.0 ** 18)
        msa.proj.weight.mul_(2.0 ** -18)
    with pytest.raises(Al3dError, match="AL3D_MATH=bf16x6"):   # the fixture really leaves the f16x3 range
        _sweep(rig, recover_range=False)
    got = _sweep(rig, recover_range=True)
    rep = dict(S.LAST_SWEEP)
    assert D.MATH == "f16x3"
    assert got.shape == (N, 512) and bool(torch.isfinite(got).all())
    assert rep["recovered_batches"] == [0, 1] and rep["recovered_frames"] == [0, 1, 2, 3], rep
    assert sorted(rep["tripped_frames"]) == [0, 1, 2, 3] and rep["batches"] == 2 and rep["math"] == "auto", rep
    ref6 = _sweep(rig, math_="bf16x6")
    assert torch.equal(_bits(got), _bits(ref6)), "recovered batches differ from the all-bf16x6 sweep"
    # the rescale is by a power of two: every bf16 piece, product and sum scales exactly
    scale = float(plain6.abs().max())
    diff = float((got - plain6).abs().max())
    print(f"rescaled vs un-rescaled model under bf16x6: max abs diff {diff:.3e} at scale {scale:.3e}; "
          f"identical bits: {torch.equal(_bits(got), _bits(plain6))}")
    assert diff <= 2e-6 * scale, (diff, scale)
    assert D.MATH == "f16x3"
