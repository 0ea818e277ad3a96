"""GPU suite: AL3D_MATH=auto -- the per-row range flag kernel, and the sweep that re-runs the batches whose f16x3
embeddings left the range under bf16x6 (bit-identical to an all-bf16x6 sweep on those rows, to a plain f16x3 sweep on
the others), in every pipeline schedule."""
import math
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda:0")
FLT_MAX = float(np.finfo(np.float32).max)

pytestmark = pytest.mark.gpu


def _bits(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------ flag kernel
@pytest.mark.parametrize("rows,cols,ld,offset", [(1, 512, 512, 0), (7, 512, 512, 0), (130, 512, 520, 0),
                                                 (128, 512, 512, 1), (33, 37, 37, 0), (65, 1, 3, 0),
                                                 (5, 513, 515, 0), (300, 61, 64, 0)])
def test_flag_kernel_matches_isfinite(rows, cols, ld, offset):
    from al3d import lib
    g = np.random.default_rng(rows * 1000 + cols)
    x = g.normal(0.0, 100.0, size=(rows, ld)).astype(np.float32)
    specials = [math.inf, -math.inf, math.nan, FLT_MAX, -FLT_MAX, 1e-40, -1e-45, 0.0]
    for r in range(rows):
        k = g.integers(0, 4)
        for _ in range(k):
            x[r, g.integers(0, cols)] = specials[g.integers(0, len(specials))]
        if ld > cols and r % 3 == 0:
            x[r, cols + g.integers(0, ld - cols)] = math.nan      # past `cols`: must not count
    x[0, cols - 1] = math.inf                                     # the last column of a row is seen
    if rows > 1:
        x[1, :cols] = FLT_MAX                                      # the largest finite values are finite
    flat = torch.empty(rows * ld + offset, dtype=torch.float32, device=DEV)
    flat[offset:] = torch.from_numpy(x.reshape(-1)).to(DEV)
    flags = torch.full((rows + 64,), 0xAB, dtype=torch.uint8, device=DEV)
    lib.call("al3d_rows_nonfinite_u8", flat.data_ptr() + 4 * offset, rows, cols, ld, flags.data_ptr(),
             torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    want = ~torch.isfinite(torch.from_numpy(x[:, :cols])).all(dim=1)
    got = flags[:rows].cpu()
    assert set(got.tolist()) <= {0, 1}
    assert torch.equal(got.bool(), want), (got.nonzero().flatten().tolist(), want.nonzero().flatten().tolist())
    assert bool((flags[rows:] == 0xAB).all()), "bytes past `rows` were written"


def test_flag_wrapper_reads_row_stride():
    from al3d import detector_ops as D
    x = torch.zeros((9, 520), dtype=torch.float32, device=DEV)
    x[:, 512:] = math.nan
    x[4, 511] = -math.inf
    got = D.rows_nonfinite(x[:, :512])
    assert got.tolist() == [0, 0, 0, 0, 1, 0, 0, 0, 0]


# ------------------------------------------------------------------ sweep recovery
@pytest.fixture(scope="module")
def rig():
    from al3d import synthetic
    from al3d.datasets import generate_task_anchors
    from al3d.models import build_detector
    from al3d.utils import Config
    cfg = Config.fromfile(os.path.join(ROOT, "examples", "active", "cbgs_spatial_temporal_feature.py"))
    anchors = generate_task_anchors(cfg.tasks, cfg.target_assigner.anchor_generators, [1, 128, 128])

    def model():
        m = build_detector(cfg.model, train_cfg=None, test_cfg=cfg.test_cfg)
        synthetic.seeded_init_(m, seed=0)
        return m
    clouds = [synthetic.make_point_cloud(500 + i, nsweeps=1) for i in range(6)]
    return dict(cfg=cfg, anchors=anchors, make_model=model, model=model().to(DEV).eval(), clouds=clouds)


def _pool(rig, hot=None, n=6):
    from al3d.datasets import PoolFrames
    clouds = [c.copy() for c in rig["clouds"][:n]]
    if hot is not None:
        clouds[hot][:, 3] = 1.0e6     # intensity: the level-0 mean-VFE input exceeds 65504
    return PoolFrames.from_numpy(clouds, DEV)


def _sweep(rig, pool, math_=None, pipeline="ahead", model=None, **kw):
    from al3d import detector_ops as D, sweep as S
    from al3d.datasets import DeviceSweepLoader
    saved = (D.MATH, S.PIPELINE)
    try:
        if math_ is not None:
            D.MATH = math_
        S.PIPELINE = pipeline
        loader = DeviceSweepLoader(pool, rig["cfg"].voxel_generator, rig["anchors"], 2, device=DEV)
        out = S.sweep_embeddings(model if model is not None else rig["model"], loader, DEV, len(pool), **kw)
        torch.cuda.synchronize()
        return out
    finally:
        D.MATH, S.PIPELINE = saved


@pytest.mark.parametrize("pipeline", [None, "ahead", "split"])
def test_auto_recovers_the_tripped_batch(rig, pipeline):
    from al3d import detector_ops as D, sweep as S
    from al3d.lib import Al3dError
    hot = _pool(rig, hot=3)
    with pytest.raises(Al3dError, match="AL3D_MATH=bf16x6"):     # the fixture really leaves the f16x3 range
        _sweep(rig, hot, pipeline=pipeline, recover_range=False)
    got = _sweep(rig, hot, pipeline=pipeline, recover_range=True)
    rep = dict(S.LAST_SWEEP)
    assert D.MATH == "f16x3"
    assert bool(torch.isfinite(got).all())
    ref6 = _sweep(rig, hot, math_="bf16x6", pipeline=pipeline)
    ref3 = _sweep(rig, _pool(rig), pipeline=pipeline)
    assert torch.equal(_bits(got[2:4]), _bits(ref6[2:4])), "recovered batch differs from the all-bf16x6 sweep"
    for r in (0, 1, 4, 5):
        assert torch.equal(_bits(got[r]), _bits(ref3[r])), f"row {r} moved"
    assert rep["recovered_batches"] == [1] and rep["tripped_frames"] == [3] and rep["recovered_frames"] == [2, 3], rep
    assert rep["batches"] == 3 and rep["math"] == "auto" and len(rep["recovery_ms"]) == 1
    print(f"pipeline={pipeline}: recovered batch of 2 frames in {rep['recovery_ms'][0]:.1f} ms of device time")


@pytest.mark.parametrize("hot,batch,with_entropy", [(0, 0, False), (5, 2, True)])
def test_auto_recovers_first_and_last_batch(rig, hot, batch, with_entropy):
    from al3d import detector_ops as D, sweep as S
    pool = _pool(rig, hot=hot)
    got = _sweep(rig, pool, recover_range=True, with_entropy=with_entropy)
    rep = dict(S.LAST_SWEEP)
    ref6 = _sweep(rig, pool, math_="bf16x6", with_entropy=with_entropy)
    rows = slice(2 * batch, 2 * batch + 2)
    if with_entropy:
        (got, ent), (ref6, ent6) = got, ref6
        # NaN included: the injected frame's mean box entropy may be NaN under bf16x6 as well (a frame without kept
        # boxes: the reference's mean over an empty set), and then it must be the same NaN
        assert torch.equal(_bits(ent[rows]), _bits(ent6[rows])), (ent[rows], ent6[rows])
        assert bool(torch.isfinite(ent[: 2 * batch]).all())
    assert bool(torch.isfinite(got).all())
    assert torch.equal(_bits(got[rows]), _bits(ref6[rows]))
    assert rep["recovered_batches"] == [batch] and rep["tripped_frames"] == [hot]
    assert rep["recovered_frames"] == [2 * batch, 2 * batch + 1]
    assert D.MATH == "f16x3"


def test_auto_without_excursion_changes_nothing(rig):
    from al3d import sweep as S
    pool = _pool(rig)
    off = _sweep(rig, pool, recover_range=False)
    on = _sweep(rig, pool, recover_range=True)
    assert S.LAST_SWEEP["recovered_batches"] == [] and S.LAST_SWEEP["tripped_frames"] == []
    assert S.LAST_SWEEP["batches"] == 3
    assert torch.equal(_bits(on), _bits(off))


def test_auto_names_frames_it_cannot_recover(rig):
    from al3d import detector_ops as D
    from al3d.lib import Al3dError
    model = rig["make_model"]()
    with torch.no_grad():
        model.neck.blocks[0][2].weight.fill_(math.inf)      # non-finite under every arithmetic
    model = model.to(DEV).eval()
    with pytest.raises(Al3dError, match=r"not recoverable.*frames \[0, 1, 2, 3\]"):
        _sweep(rig, _pool(rig, n=4), model=model, recover_range=True)
    assert D.MATH == "f16x3"
