"""CPU suite for the box-wise IoU estimator: the registry and builder names, the reference's parameter names, the float64
restatement tests/estimator_numpy.py against the reference's own run recorded in tests/golden/estimator.npz
(tools/gen_golden_estimator.py), and the pieces that need no device.

Tolerance of the IoUs: 4 x ``ref_f32_gap``, the reference's own float32 distance from float64 on this fixture as stored in
the file; float64 against the reference's float32 cannot be asked to do better than the reference's own rounding, the
factor allows for the summation order of a restated matmul.  Counts and survivors are exact: the generator keeps every
point at least 1e-3 m from every membership boundary."""
import os

import numpy as np
import pytest
import torch

import estimator_numpy as EN

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
TASKS = [dict(num_class=4, class_names=["a", "b", "c", "d"]), dict(num_class=6, class_names=list("efghij"))]


@pytest.fixture(scope="module")
def z():
    return np.load(os.path.join(GOLDEN, "estimator.npz"), allow_pickle=False)


@pytest.fixture(scope="module")
def yard(z):
    state = {k[6:]: z[k] for k in z.files if k.startswith("state.")}
    return EN.run(z["boxes"], z["labels"], z["counts"], z["points"], z["offsets"], state, int(z["num_classes"]))


def test_registry_and_builder():
    from al3d.models import ESTIMATORS, build_estimator
    from al3d.models.estimator import Estimator
    assert ESTIMATORS.get("Estimator") is Estimator
    m = build_estimator(dict(type="Estimator", tasks=TASKS, dim_feat=224))
    assert isinstance(m, Estimator) and m.num_classes == 10 and m.num_tasks == 2 and m.dim_feat == 224
    assert [tuple(l.weight.shape) for l in m.iou_estimator if isinstance(l, torch.nn.Linear)] == [(32, 19), (64, 32), (128, 64)]
    assert [tuple(l.weight.shape) for l in m.iou_head if isinstance(l, torch.nn.Linear)] == [(256, 128), (64, 256), (1, 64)]


def test_golden_state_dict_loads_strict(z):
    from al3d.models import build_estimator
    m = build_estimator(dict(type="Estimator", tasks=TASKS, dim_feat=224))
    state = {k[6:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("state.")}
    assert sorted(state) == sorted(m.state_dict())
    m.load_state_dict(state, strict=True)
    names = {k.rsplit(".", 1)[0] for k in state}
    assert names == {f"iou_estimator.{i}" for i in (0, 1, 3, 4, 6, 7)} | {f"iou_head.{i}" for i in (0, 1, 3, 4, 6)}


def test_fixture_shapes(z):
    """The cases the fixture is there for (the generator asserts them too, on the restatement)."""
    assert z["boxes"].shape == (4, 2, 8, 9) and int(z["num_classes"]) == 10
    assert np.diff(z["offsets"]).tolist() == [1300, 70, 0, 1300]
    assert sorted(set(z["counts"].ravel().tolist())) == [0, 1, 8]
    n0 = z["ref_npts"][0]
    assert n0[0, 2] == 1 and n0[0, 4] == 0                  # one point; in the footprint but outside the height
    assert n0[0, 5] == 1 and n0[0, 6] == 0                  # the rotation quirk: inside / outside for that reason alone
    assert float(z["dropped_share"]) <= 0.05 and float(z["ref_f32_gap"]) > 0
    ang = z["boxes"][..., 6]
    assert ang.min() < -np.pi and ang.max() > np.pi


def test_rotation_quirk_is_pinned(z):
    """Frame 0, task 0, boxes 5 and 6 (w = 1, l = 3, angle 0.8) each have one point nearby, at FEATURE-frame offset
    (1.1 w, 0) and (0, 0.9 l).  Were the footprint rotated in the feature frame's sense, the first would be outside
    (1.1 w > w) and the second inside (0.9 l < l); the reference has it the other way round."""
    pts = z["points"][:1300].astype(np.float64)
    for i, want, loc in ((5, True, (1.1, 0.0)), (6, False, (0.0, 2.7))):
        box = z["boxes"][0, 0, i]
        near = np.nonzero(np.hypot(pts[:, 0] - box[0], pts[:, 1] - box[1]) < 4.0)[0]
        f = EN.features(pts[near], box, 0, 10)
        k = int(np.argmin(np.abs(f[:, 0] - loc[0]) + np.abs(f[:, 1] - loc[1]) + np.abs(f[:, 2])))
        assert np.allclose(f[k, :3], [loc[0], loc[1], 0.0], atol=1e-5)
        assert bool(EN.inside(pts[near[k]][None], box)[0]) is want
        agree = (abs(loc[0]) < box[3]) and (abs(loc[1]) < box[4])       # membership if both rotations agreed
        assert agree is not want


def test_numpy_reproduces_the_reference(z, yard):
    assert np.array_equal(yard["npts"], z["ref_npts"])
    assert np.array_equal(yard["counts"], z["ref_out_counts"])
    mask = np.zeros(z["ref_survivor_mask"].shape, dtype=bool)
    for bt, keep in enumerate(yard["survivors"]):
        mask[bt // 2, bt % 2, keep] = True
    assert np.array_equal(mask, z["ref_survivor_mask"])
    tol = 4 * float(z["ref_f32_gap"])
    assert np.array_equal(np.isnan(yard["iou"]), np.isnan(z["ref_iou"]))
    ok = ~np.isnan(z["ref_iou"])
    gap = np.abs(yard["iou"][ok] - z["ref_iou"][ok].astype(np.float64)).max()
    print(f"max |f64 - reference f32| IoU {gap:.3e}, tolerance {tol:.3e}")
    assert gap <= tol
    assert np.array_equal(yard["iou"][ok], z["f64_iou"][ok])
    # the sampled feature rows, to float32 rounding of values of a few metres
    f = np.stack([EN.features(z["points"][z["offsets"][b] + p][None], z["boxes"][b, t, i], z["labels"][b, t, i], 10)[0]
                  for b, t, i, p in z["feat_pairs"]])
    assert np.abs(f - z["ref_features"]).max() < 1e-5
    assert (z["ref_features"][:, 3:9].min(axis=1) < 0).any()            # the ring: negative centerness


def test_fold_matches_eval_batchnorm(z):
    from al3d.models import build_estimator
    from al3d.models.estimator import fold_linear_bn
    m = build_estimator(dict(type="Estimator", tasks=TASKS, dim_feat=0)).eval()
    m.load_state_dict({k[6:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("state.")})
    x = torch.randn(50, 19, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    w, b = fold_linear_bn(m.iou_estimator[0], m.iou_estimator[1])
    ref = m.double().iou_estimator[:2](x)
    assert torch.allclose(x @ w.double().t() + b.double(), ref, atol=1e-6)
    packed = m.float().packed_weights("cpu")
    assert packed.numel() == 32 * 19 + 32 + 64 * 32 + 64 + 128 * 64 + 128 + 128 * 256 + 256 + 256 * 64 + 64 + 64 + 1
    assert m.packed_weights("cpu") is packed                # the cache holds it until a parameter changes
    m.load_state_dict(m.state_dict())
    assert m.packed_weights("cpu") is not packed


def test_return_loss_raises():
    from al3d.models import build_estimator
    from al3d.models.estimator import WithEstimator
    m = build_estimator(dict(type="Estimator", tasks=TASKS, dim_feat=224)).eval()
    with pytest.raises(NotImplementedError, match="inference sweep, not training"):
        m(dict(preds=[], points=torch.zeros(0, 5)), return_loss=True)
    with pytest.raises(NotImplementedError, match="inference sweep, not training"):
        WithEstimator(torch.nn.Identity(), m)(dict(), return_loss=True)


def test_too_many_classes_refused():
    from al3d.lib import Al3dError
    from al3d.models import build_estimator
    with pytest.raises(Al3dError):
        build_estimator(dict(type="Estimator", tasks=[dict(class_names=[str(i) for i in range(33)])], dim_feat=0))


def test_abi_refuses_bad_sizes_before_any_launch():
    from al3d import lib
    so = lib.load()
    assert so.al3d_estimator_workspace_bytes(4, 2, 8) > 0
    assert so.al3d_estimator_workspace_bytes(1, 2, 513) == -1          # nt * post above AL3D_EST_MAX_BOXES
    assert so.al3d_estimator_weight_elems(10) == 60609 and so.al3d_estimator_weight_elems(33) == -1
    p = 256
    rc = so.al3d_estimator_f32(p, p, p, 1, 2, 513, 9, 6, p, p, 10, 5, p, 60609, 10, p, p, p, p, p, p, None)
    assert rc == -1 and b"at most 1024" in so.al3d_last_error()
    rc = so.al3d_estimator_f32(p, p, p, 1, 2, 8, 9, 6, p, p, 10, 5, p, 60609, 33, p, p, p, p, p, p, None)
    assert rc == -1 and b"num_classes" in so.al3d_last_error()
    rc = so.al3d_estimator_f32(p, p, p, 1, 2, 8, 9, 6, p, p, 10, 5, p, 100, 10, p, p, p, p, p, p, None)
    assert rc == -1 and b"packed weights" in so.al3d_last_error()


def test_device_loader_keeps_points_only_when_asked():
    """``keep_points`` is off by default and the default batch has no ``points`` key (checked on the loader's source: a
    batch itself needs the device voxelizer)."""
    import inspect
    from al3d.datasets import DeviceSweepLoader
    sig = inspect.signature(DeviceSweepLoader.__init__)
    assert sig.parameters["keep_points"].default is False
    src = inspect.getsource(DeviceSweepLoader.__iter__)
    head, tail = src.split("if self.keep_points:")
    assert '"points"' not in head and 'ex["points"], ex["point_offsets"] = pts, off' in tail
