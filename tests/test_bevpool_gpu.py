"""GPU suite, SURVEY section 8 row f4 (camera branch, first slice): al3d_bev_pool_f32 / al3d_bev_pool_lss_f32 through
the C ABI against the oracle (bit-exact: both sum a cell's points in ascending index order), the Lift-Splat view
transform + ConvFuser modules against torch fp32 convolutions, and a full-size camera + lidar fusion pass
(6 x 118 x 32 x 88 frustum points, 360 x 360 BEV cells, 80 + 256 -> 256 channels at 180 x 180) for determinism.
Reference: bevfusion/mmdet3d/models/vtransforms/base.py:56-163, depth_lss.py:58-102, fusers/conv.py:11-25,
ops/bev_pool/src/bev_pool_cuda.cu:21-44 (needs bev_pool_ext + mmcv: parity unpinned, oracle pinned by a torch
index_add_ statement in tests/test_bevpool_oracle.py)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.mark.parametrize("C", [80, 6, 128, 256, 4])          # float4 lane groups (3 / 2 / 1 / 4 cells per wave) and the generic kernel (6)
@pytest.mark.parametrize("case", ["random", "crowded", "empty", "all_outside"])
def test_bev_pool_bit_exact_vs_oracle(oracle, case, C):
    from al3d.models.bevfusion_camera import bev_pool
    rng = np.random.default_rng(5)
    B = 2
    nx, dx, bx = np.array([24, 20, 2]), np.array([0.5, 0.5, 4.0], np.float32), np.array([-5.75, -4.75, -2.0], np.float32)
    P = {"random": 40000, "crowded": 9000, "empty": 0, "all_outside": 64}[case]
    geom = np.stack([rng.uniform(-7, 7, P), rng.uniform(-6, 6, P), rng.uniform(-5, 5, P)], 1).astype(np.float32)
    if case == "crowded":                    # thousands of points in a handful of cells: lists far beyond one wave
        geom[:, 0] = rng.choice([-5.9, -5.4, 0.1], P)
        geom[:, 1] = rng.choice([-4.9, 0.2], P)
        geom[:, 2] = -1.0
    if case == "all_outside":
        geom[:] = 100.0
    x = rng.normal(size=(P, C)).astype(np.float32)
    lo = bx - dx / np.float32(2)
    ref = oracle.bev_pool(x, geom, B, lo, dx, nx)
    got = bev_pool(_t(x), _t(geom), B, dx, bx, nx)
    got2 = bev_pool(_t(x), _t(geom), B, dx, bx, nx)
    assert got.shape == (B, 24, 20, 2 * C) and torch.equal(got, got2)       # run-to-run bitwise
    assert np.array_equal(got.cpu().numpy().view(np.int32), ref.view(np.int32))
    if case in ("random", "crowded"):
        assert np.abs(ref).sum() > 0


def test_bev_pool_fused_lss_bit_exact(oracle):
    from al3d.models.bevfusion_camera import bev_pool
    rng = np.random.default_rng(6)
    B, N, D, fH, fW, C = 2, 3, 7, 6, 10, 80
    depth = rng.uniform(0, 1, (B * N, D, fH, fW)).astype(np.float32)
    ctx = rng.normal(size=(B * N, fH, fW, C)).astype(np.float32)
    geom = rng.uniform(-6, 6, (B * N * D * fH * fW, 3)).astype(np.float32)
    nx, dx, bx = np.array([30, 30, 1]), np.array([0.4, 0.4, 20.0], np.float32), np.array([-5.8, -5.8, 0.0], np.float32)
    lo = bx - dx / np.float32(2)
    ref = oracle.bev_pool(ctx.reshape(-1, C), geom, B, lo, dx, nx, depth=depth.reshape(-1), D=D, fHW=fH * fW)
    got = bev_pool(_t(ctx), _t(geom), B, dx, bx, nx, depth=_t(depth)).cpu().numpy()
    assert np.array_equal(got.view(np.int32), ref.view(np.int32))
    mat = bev_pool(_t((depth[..., None] * ctx[:, None]).reshape(-1, C)), _t(geom), B, dx, bx, nx).cpu().numpy()
    assert np.array_equal(got.view(np.int32), mat.view(np.int32))           # fused == materialised (depth_lss.py:93)


def _calib(B, N, rng):
    """nuScenes-like rig: N cameras looking outward, 900x1600 images resized/cropped to 256x704."""
    rots, trans, intr, prot, ptr_ = [], [], [], [], []
    for b in range(B):
        for n in range(N):
            yaw = 2 * np.pi * n / N + rng.normal(0, 0.02)
            # camera axes (x right, y down, z forward) -> lidar axes (x forward at yaw, y left, z up)
            fwd = np.array([np.cos(yaw), np.sin(yaw), 0.0])
            right = np.array([np.sin(yaw), -np.cos(yaw), 0.0])
            down = np.array([0.0, 0.0, -1.0])
            rots.append(np.stack([right, down, fwd], 1))
            trans.append(np.array([1.5 * np.cos(yaw), 1.5 * np.sin(yaw), 1.6]))
            intr.append(np.array([[1266.0, 0, 816.0], [0, 1266.0, 491.0], [0, 0, 1.0]]))
            s = 0.48
            prot.append(np.diag([s, s, 1.0]))
            ptr_.append(np.array([-32.0, -176.0, 0.0]))
    f = lambda a, *sh: torch.tensor(np.asarray(a), dtype=torch.float32).view(B, N, *sh).to(DEV)
    return f(rots, 3, 3), f(trans, 3), f(intr, 3, 3), f(prot, 3, 3), f(ptr_, 3)


def test_lss_view_transform_and_fuser_vs_torch(oracle):
    from al3d import synthetic
    from al3d.models.bevfusion_camera import ConvFuser, LSSViewTransform
    rng = np.random.default_rng(7)
    B, N, C = 1, 2, 16
    vt = LSSViewTransform(C, image_size=(64, 96), feature_size=(8, 12), xbound=(-12.0, 12.0, 0.5), ybound=(-12.0, 12.0, 0.5),
                          zbound=(-10.0, 10.0, 20.0), dbound=(1.0, 13.0, 1.0), downsample=2)
    fuser = ConvFuser([C, 32], 48)
    synthetic.seeded_init_(vt.downsample, seed=1)
    synthetic.seeded_init_(fuser, seed=2)
    vt, fuser = vt.to(DEV).eval(), fuser.to(DEV).eval()
    rots, trans, intr, prot, ptr_ = _calib(B, N, rng)
    prot = prot * 0 + torch.eye(3, device=DEV) * 0.06
    prot[..., 2, 2] = 1.0
    ptr_ = ptr_ * 0
    Dd = vt.D
    depth = torch.softmax(torch.randn(B, N, Dd, 8, 12, device=DEV), dim=2)
    ctx = torch.randn(B, N, 8, 12, C, device=DEV)
    with torch.no_grad():
        cam = vt(depth, ctx, rots, trans, intr, prot, ptr_)
        # torch statement: materialise, pool with the oracle on the same geometry, convs with F.conv2d
        # geometry: the device kernel against the reference's torch expressions (base.py:79-122)
        gd = vt.geometry_device(rots, trans, intr, prot, ptr_)
        torch.testing.assert_close(gd, vt.get_geometry(rots, trans, intr, prot, ptr_), rtol=1e-5, atol=1e-4)
        er = torch.tensor([[[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]], device=DEV)
        et = torch.tensor([[0.5, -0.25, 0.1]], device=DEV)
        torch.testing.assert_close(vt.geometry_device(rots, trans, intr, prot, ptr_, extra_rots=er, extra_trans=et),
                                   vt.get_geometry(rots, trans, intr, prot, ptr_, extra_rots=er, extra_trans=et),
                                   rtol=1e-5, atol=1e-4)
        geom = gd.reshape(-1, 3).cpu().numpy()
        x = (depth.unsqueeze(-1) * ctx.unsqueeze(2)).reshape(-1, C).cpu().numpy()
        lo = vt.bx.cpu().numpy() - vt.dx.cpu().numpy() / np.float32(2)
        pooled = torch.from_numpy(oracle.bev_pool(x, geom, B, lo, vt.dx.cpu().numpy(), vt.nx.cpu().numpy()))
        assert float(pooled.abs().sum()) > 0
        ref = vt.downsample.cpu()(pooled.permute(0, 3, 1, 2)).permute(0, 2, 3, 1)
        vt.downsample.to(DEV)
        torch.testing.assert_close(cam.cpu(), ref, rtol=1e-4, atol=1e-4)
        lidar = torch.randn(B, cam.shape[1], cam.shape[2], 32, device=DEV)
        fused = fuser([cam, lidar])
        want = nn_seq_nchw(fuser, torch.cat([cam, lidar], -1))
        torch.testing.assert_close(fused.cpu(), want, rtol=1e-4, atol=1e-4)
    assert cam.shape == (B, 24, 24, C) and fused.shape == (B, 24, 24, 48)


def nn_seq_nchw(seq, x_nhwc):
    """Run conv + BN(eval) + ReLU of an nn.Sequential with torch CPU fp32 ops on a channels-last input."""
    conv, bn = seq[0], seq[1]
    y = F.conv2d(x_nhwc.cpu().permute(0, 3, 1, 2), conv.weight.cpu(), stride=conv.stride, padding=conv.padding)
    y = F.batch_norm(y, bn.running_mean.cpu(), bn.running_var.cpu(), bn.weight.cpu(), bn.bias.cpu(), False, 0.0, bn.eps)
    return torch.relu(y).permute(0, 2, 3, 1)


def test_full_size_camera_lidar_fusion_pass(oracle):
    """configs[4] shapes: 6 cameras, 118 depth bins, 32 x 88 feature maps, 80 channels -> 360 x 360 BEV cells ->
    downsample 2 -> ConvFuser with a 256-channel lidar BEV map at 180 x 180 -> SECOND/SECONDFPN decoder (the RPN module)
    -> 512-d embedding.  The whole pass: determinism and finiteness (no reference for the conv stacks at this size).  The
    fused pooling alone -- 1,993,728 frustum points, lists from 0 to about 1,000 members side by side as the real rig
    produces them -- bit for bit against the CPU oracle on the downloaded geom / depth / ctx (half a second on the host),
    besides the float64 total-mass check, which one lost or repeated point out of 2 M would pass."""
    import time
    from al3d import detector_ops as D, synthetic
    from al3d.models.bevfusion_camera import ConvFuser, LSSViewTransform
    from al3d.models.necks import RPN
    rng = np.random.default_rng(8)
    B, N, C = 1, 6, 80
    vt = LSSViewTransform(C, image_size=(256, 704), feature_size=(32, 88), xbound=(-54.0, 54.0, 0.3),
                          ybound=(-54.0, 54.0, 0.3), zbound=(-10.0, 10.0, 20.0), dbound=(1.0, 60.0, 0.5), downsample=2)
    fuser = ConvFuser([80, 256], 256)
    dec = RPN(layer_nums=[5, 5], ds_layer_strides=[1, 2], ds_num_filters=[128, 256], us_layer_strides=[1, 2],
              us_num_filters=[256, 256], num_input_features=256)
    for i, m in enumerate((vt.downsample, fuser, dec)):
        synthetic.seeded_init_(m, seed=10 + i)
    vt, fuser, dec = vt.to(DEV).eval(), fuser.to(DEV).eval(), dec.to(DEV).eval()
    assert vt.D == 118 and vt.nx.tolist() == [360, 360, 1]
    rots, trans, intr, prot, ptr_ = _calib(B, N, rng)
    depth = torch.softmax(torch.randn(B, N, 118, 32, 88, device=DEV), dim=2)
    ctx = torch.randn(B, N, 32, 88, C, device=DEV) * 0.5
    lidar = torch.relu(torch.randn(B, 180, 180, 256, device=DEV))

    def run():
        with torch.no_grad():
            cam = vt(depth, ctx, rots, trans, intr, prot, ptr_)
            return cam, D.gap_nhwc(dec(fuser([cam, lidar])))
    cam, emb = run()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    cam2, emb2 = run()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    assert cam.shape == (1, 180, 180, 80) and emb.shape == (1, 512)
    assert torch.isfinite(emb).all() and torch.equal(emb, emb2) and torch.equal(cam, cam2)
    # pooling alone: total mass of the pooled map == sum of depth * ctx over the kept points (float64)
    from al3d.models.bevfusion_camera import bev_pool
    geom = vt.geometry_device(rots, trans, intr, prot, ptr_)
    pooled = bev_pool(ctx.reshape(B * N, 32, 88, C).contiguous(), geom.contiguous(), B, vt.dx.cpu().numpy(),
                      vt.bx.cpu().numpy(), vt.nx.cpu().numpy(), depth=depth.reshape(B * N, 118, 32, 88).contiguous())
    lo = (vt.bx - vt.dx / 2.0)
    cell = ((geom - lo) / vt.dx).long()
    kept = ((cell >= 0) & (cell < vt.nx)).all(-1)                        # [B,N,D,fH,fW]
    want = (depth.double() * kept.double()).unsqueeze(-1) * ctx.double().unsqueeze(2)
    assert abs(float(pooled.double().sum()) - float(want.sum())) <= 1e-6 * float(want.abs().sum())
    assert 0.2 < float(kept.float().mean()) <= 1.0
    t0 = time.perf_counter()
    geom_h, depth_h, ctx_h = geom.reshape(-1, 3).cpu().numpy(), depth.reshape(-1).cpu().numpy(), ctx.reshape(-1, C).cpu().numpy()
    lo_h = vt.bx.cpu().numpy().astype(np.float32) - vt.dx.cpu().numpy().astype(np.float32) / np.float32(2)
    ref = oracle.bev_pool(ctx_h, geom_h, B, lo_h, vt.dx.cpu().numpy(), vt.nx.cpu().numpy(), depth=depth_h, D=118, fHW=32 * 88)
    same = (pooled.cpu().numpy().view(np.int32) == ref.view(np.int32)).reshape(-1, C).all(-1)
    per_cell = torch.bincount(((cell[..., 0] * 360 + cell[..., 1])[kept]).reshape(-1), minlength=360 * 360)
    assert same.all(), f"{int((~same).sum())} of {same.size} cells differ from the oracle, first ids {np.flatnonzero(~same)[:8].tolist()}"
    assert int(per_cell.max()) > 128 and int((per_cell == 0).sum()) > 0          # sorted lists next to short and empty ones
    print(f"full-size fused pooling == oracle bit for bit ({time.perf_counter() - t0:.2f} s for download + oracle + compare; "
          f"longest member list {int(per_cell.max())})")
    print(f"camera+lidar fusion pass at configs[4] shapes: {dt * 1e3:.1f} ms per sample "
          f"({int(kept.sum())} of {kept.numel()} frustum points inside the grid)")


@pytest.mark.parametrize("C", [6, 260])
def test_bev_pool_fused_lss_generic_kernel_bit_exact(oracle, C):
    """The fused Lift-Splat pooling at channel counts the float4 kernel does not take (C % 4 != 0; C / 4 > 64):
    bev_sum_kernel<1>, against the oracle and against pooling the materialised depth x context rows."""
    from al3d.models.bevfusion_camera import bev_pool
    rng = np.random.default_rng(60 + C)
    B, N, D, fH, fW = 2, 3, 7, 6, 10
    depth = rng.uniform(0, 1, (B * N, D, fH, fW)).astype(np.float32)
    ctx = rng.normal(size=(B * N, fH, fW, C)).astype(np.float32)
    geom = rng.uniform(-6, 6, (B * N * D * fH * fW, 3)).astype(np.float32)
    nx, dx, bx = np.array([30, 30, 1]), np.array([0.4, 0.4, 20.0], np.float32), np.array([-5.8, -5.8, 0.0], np.float32)
    lo = bx - dx / np.float32(2)
    ref = oracle.bev_pool(ctx.reshape(-1, C), geom, B, lo, dx, nx, depth=depth.reshape(-1), D=D, fHW=fH * fW)
    got = bev_pool(_t(ctx), _t(geom), B, dx, bx, nx, depth=_t(depth)).cpu().numpy()
    assert np.abs(ref).sum() > 0 and np.array_equal(got.view(np.int32), ref.view(np.int32))
    mat = bev_pool(_t((depth[..., None] * ctx[:, None]).reshape(-1, C)), _t(geom), B, dx, bx, nx).cpu().numpy()
    assert np.array_equal(got.view(np.int32), mat.view(np.int32))
