"""Bits and launches of every module that packs convolution weights, for an A/B of two trees on one library.

  python tools/ab_module_bits.py --out run.json            # hashes + steady-state launch lists, f16x3 and bf16x6
  python tools/ab_module_bits.py --host-cost               # host time of RPN / MultiGroupHead / encoder ``_prepare``
  python tools/ab_module_bits.py --compare a.json b.json   # exit status 1 if any hash or launch list differs

Seeded weights and inputs.  Per module and arithmetic: SHA-256 of every output tensor of the second forward, and the ordered
entry-point names ``lib.call`` saw during it (the first forward packs).  The tool only uses what both sides of a refactor of
the packing layer share: the registries' builders and the modules' forward methods."""
import argparse
import hashlib
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEV = "cuda:0"


def sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()[:16]


def randn(*shape, seed=0, scale=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).to(DEV)


def voxels(batch, grid, per_frame, channels, seed):
    """Random distinct sites of a [batch, *grid] grid, frame by frame: (features [N, channels], coords [N, 4] i32)."""
    g = torch.Generator().manual_seed(seed)
    cells = grid[0] * grid[1] * grid[2]
    rows = []
    for b in range(batch):
        flat = torch.randperm(cells, generator=g)[:per_frame]
        z, y, x = flat // (grid[1] * grid[2]), flat // grid[2] % grid[1], flat % grid[2]
        rows.append(torch.stack([torch.full_like(z, b), z, y, x], 1))
    coords = torch.cat(rows).to(torch.int32)
    return torch.randn(coords.shape[0], channels, generator=g).to(DEV), coords.to(DEV)


def sections():
    """name -> (build() -> run, where run() -> {output name: tensor})."""
    from al3d import synthetic
    from al3d.models import build_backbone, build_head, build_neck, build_reader
    from al3d.utils import Config
    cfg = Config.fromfile(os.path.join(ROOT, "examples", "active", "cbgs_spatial_temporal_feature.py"))

    def rpn_head():
        neck = synthetic.seeded_init_(build_neck(cfg.model.neck), 1).to(DEV).eval()
        head = synthetic.seeded_init_(build_head(cfg.model.bbox_head), 2).to(DEV).eval()
        x = randn(1, 128, 128, cfg.model.neck.num_input_features, seed=3)

        def run():
            y = neck(x)
            return dict(neck=y, embedding=neck.embedding if neck.embedding is not None else y[:0], head=head(y)[0]["_fused"])
        return run, dict(neck=neck, head=head)

    def encoder():
        enc = synthetic.seeded_init_(build_backbone(cfg.model.backbone), 4).to(DEV).eval()
        feats, coords = voxels(2, (41, 128, 128), 6000, cfg.model.backbone.num_input_features, 5)

        def run():
            dense, middle = enc(feats, coords, 2, [128, 128, 40])
            return dict(dense=dense, **{f"stage{i}": m.features for i, m in enumerate(middle)})
        return run, dict(encoder=enc, coords=coords)

    def decoder():
        net = synthetic.seed_modules_(build_backbone(dict(type="GeneralizedResNet", in_channels=80,
                                                          blocks=[[2, 128, 2], [2, 256, 2], [2, 512, 1]])), 1).to(DEV).eval()
        fpn = synthetic.seed_modules_(build_neck(dict(type="LSSFPN", in_indices=[-1, 0], in_channels=[512, 128],
                                                      out_channels=256, scale_factor=2)), 2).to(DEV).eval()
        x = randn(1, 128, 128, 80, seed=6)
        return (lambda: dict(out=fpn(net(x)))), {}

    def view_transform():
        from al3d.models.bevfusion_camera import DepthLSSTransform
        vt = DepthLSSTransform(256, 80, (256, 704), (32, 88), [-54.0, 54.0, 0.3], [-54.0, 54.0, 0.3], [-10.0, 10.0, 20.0],
                               [1.0, 60.0, 0.5], downsample=2)
        vt = synthetic.seed_modules_(vt, 3).to(DEV).eval()
        d, y, x = randn(6, 256, 704, 1, seed=7).abs(), randn(6, 32, 88, 320, seed=8), randn(1, 360, 360, 80, seed=9)

        def chain(layers, t):
            for layer in layers:
                t = layer(t)
            return t
        return (lambda: dict(dtransform=chain(vt._dt, d), dtransform01=vt._dtransform01(d[..., 0].contiguous()),
                             depthnet=chain(vt._dn, y), downsample=chain(vt._ds, x))), {}

    def center_head():
        head = build_head(dict(
            type="CenterHead", in_channels=32, share_conv_channel=64, norm_bbox=True, transpose_input=True,
            tasks=[["car"], ["truck", "construction_vehicle"], ["pedestrian", "traffic_cone"]],
            common_heads=dict(reg=[2, 2], height=[1, 2], dim=[3, 2], rot=[2, 2], vel=[2, 2]),
            separate_head=dict(type="SeparateHead", init_bias=-2.19, final_kernel=3)))
        head = synthetic.seeded_init_(head, 10).to(DEV).eval()
        x = randn(2, 32, 32, 32, seed=11)
        return (lambda: dict(fused=head(x).fused)), {}

    def transfusion_convs():
        from al3d.models.transfusion_head import TransFusionHead
        head = TransFusionHead(
            num_proposals=200, auxiliary=True, in_channels=512, hidden_channel=128, num_classes=10, num_decoder_layers=1,
            num_heads=8, nms_kernel_size=3, ffn_channel=256, dropout=0.1, bn_momentum=0.1, activation="relu",
            common_heads=dict(center=[2, 2], height=[1, 2], dim=[3, 2], rot=[2, 2], vel=[2, 2]),
            test_cfg=dict(dataset="nuScenes", grid_size=[512, 512, 1], out_size_factor=8, voxel_size=[0.075, 0.075],
                          pc_range=[-54.0, -54.0], nms_type=None),
            bbox_coder=dict(pc_range=[-54.0, -54.0], post_center_range=[-61.2, -61.2, -10.0, 61.2, 61.2, 10.0],
                            score_threshold=0.0, out_size_factor=8, voxel_size=[0.075, 0.075], code_size=10))
        head = synthetic.seed_modules_(head, 12).to(DEV).eval()
        x = randn(1, 32, 32, 512, seed=13)

        def run():
            lidar = head._convs[0](x)
            return dict(shared=lidar, heatmap=head._convs[2](head._convs[1](lidar)))
        return run, {}

    def seg_head():
        head = build_head(dict(type="BEVSegmentationHead", in_channels=32, loss="focal",
                               grid_transform=dict(input_scope=[[-6.0, 6.0, 1.0], [-10.0, 10.0, 1.0]],
                                                   output_scope=[[-7.5, 6.7, 0.7], [-11.6, 9.0, 0.9]]),
                               classes=["drivable_area", "ped_crossing", "walkway", "stop_line", "carpark_area", "divider"]))
        head = synthetic.seed_modules_(head, 14).to(DEV).eval()
        x = randn(2, 12, 20, 32, seed=15)
        return (lambda: dict(prob=head(x))), {}

    def pillar_reader():
        reader = synthetic.seeded_init_(build_reader(dict(type="PillarFeatureNet", num_input_features=5, num_filters=[64])),
                                        16).to(DEV).eval()
        g = torch.Generator().manual_seed(17)
        M, P = 3000, 20
        feats = torch.randn(M, P, 5, generator=g).to(DEV)
        num = torch.randint(1, P + 1, (M,), generator=g).to(torch.int32).to(DEV)
        _, coords = voxels(1, (1, 128, 128), M, 1, 18)
        return (lambda: dict(rows=reader(feats, num, coords))), {}

    def spconv_net():
        from torch import nn
        from al3d import spconv
        net = spconv.SparseSequential(
            spconv.SubMConv3d(16, 16, 3, indice_key="a"), nn.BatchNorm1d(16), nn.ReLU(),
            spconv.SparseConv3d(16, 32, 3, 2, padding=1), nn.BatchNorm1d(32), nn.ReLU(),
            spconv.SubMConv3d(32, 32, 3, indice_key="b"), nn.BatchNorm1d(32), nn.ReLU())
        net = synthetic.seeded_init_(net, 19).to(DEV).eval()
        feats, coords = voxels(2, (16, 48, 48), 3000, 16, 20)

        def run():
            out = net(spconv.SparseConvTensor(feats, coords, [16, 48, 48], 2))
            return dict(features=out.features, indices=out.indices)
        return run, {}

    def swin_t():
        """Swin-T on a map that needs padding (patch embedding, the fused attention block and MLP at embed 96 and 192, the
        token GEMMs of the wider stages), and the token GEMM with pair rows in and out, which no module asks for."""
        from al3d import detector_ops as D, token_ops as T
        from al3d.models.swin import SwinTransformer
        swin = synthetic.seed_modules_(SwinTransformer(embed_dims=96, depths=[2, 2, 6, 2], num_heads=[3, 6, 12, 24], window_size=7,
                                                       mlp_ratio=4, qkv_bias=True, patch_norm=True, out_indices=[1, 2, 3]), 23)
        swin = swin.to(DEV).eval()
        img = randn(2, 96, 160, 3, seed=21)
        a, pk = randn(300, 192, seed=22), T.PackedLinear(randn(136, 192, seed=24, scale=192 ** -0.5), randn(136, seed=25))

        def run():
            out = {f"level{i}": o for i, o in enumerate(swin(img))}
            if D.MATH == "f16x3":
                out["linear_pair_pair"] = T.linear(D.rows_convert(a, True), pk, a_pair=True, act="gelu", out_pair=True)
            return out
        return run, {}

    def opt_in_dense():
        """The f16x3 dense kernels no default dispatch reaches: the fused residual 3x3 (AL3D_RES=fused) and Winograd."""
        from al3d import detector_ops as D
        if D.MATH != "f16x3":
            return (lambda: {}), {}
        x, res = randn(2, 21, 37, 64, seed=26), randn(2, 21, 37, 128, seed=27)
        w, bs, bt = randn(128, 9, 64, seed=28, scale=1.0 / 24), randn(128, seed=29).abs() + 0.5, randn(128, seed=30)
        wr, sr = D.pack_res3x3(w, bs)
        ww, sw = D.pack_wino_f16x3(w, bs)
        return (lambda: dict(res3x3=D.conv3x3_res_nhwc(x, wr, sr, bt, res),
                             wino=D.conv2d_nhwc(x, ww, sw, bt, 3, 1, 1, True),
                             wino_pair=D.conv2d_nhwc(x, ww, sw, bt, 3, 1, 1, True, io=D.IO_OUT_PAIR))), {}

    return dict(rpn_head=rpn_head, encoder=encoder, decoder=decoder, view_transform=view_transform, center_head=center_head,
                transfusion_convs=transfusion_convs, seg_head=seg_head, pillar_reader=pillar_reader, spconv_net=spconv_net,
                swin_t=swin_t, opt_in_dense=opt_in_dense)


def record(out_path):
    from al3d import detector_ops as D, lib
    real_call, names = lib.call, []

    def call(name, *args):
        names.append(name)
        return real_call(name, *args)
    lib.call = call
    results = {}
    default = D.MATH
    try:
        for math in ("f16x3", "bf16x6"):
            D.MATH = math
            for name, build in sections().items():
                with torch.no_grad():
                    run, _ = build()
                    run()
                    torch.cuda.synchronize()
                    del names[:]
                    out = run()
                    launches = list(names)
                torch.cuda.synchronize()
                results[f"{name}/{math}"] = dict(hashes={k: sha(v) for k, v in out.items()}, launches=launches)
                print(name, math, len(launches), "launches", flush=True)
    finally:
        D.MATH, lib.call = default, real_call
    with open(out_path, "w") as f:
        json.dump(results, f, indent=1, sort_keys=True)


def host_cost(calls=1000):
    """us per ``_prepare`` call, second call onwards, of the three modules whose stamp walks many layers."""
    made = sections()
    with torch.no_grad():
        run, mods = made["rpn_head"]()
        run()
        enc_run, enc = made["encoder"]()
        enc_run()
    todo = dict(RPN=lambda: mods["neck"]._prepare(torch.device(DEV)), MultiGroupHead=lambda: mods["head"]._prepare(torch.device(DEV)),
                encoder=lambda: enc["encoder"]._prepare(enc["coords"].device))
    for name, fn in todo.items():
        fn()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        print(f"{name}._prepare: {(time.perf_counter() - t0) / calls * 1e6:.1f} us per call ({calls} calls)", flush=True)


def compare(a_path, b_path):
    with open(a_path) as f:
        a = json.load(f)
    with open(b_path) as f:
        b = json.load(f)
    bad = 0
    for key in sorted(set(a) | set(b)):
        ra, rb = a.get(key), b.get(key)
        same_h = ra is not None and rb is not None and ra["hashes"] == rb["hashes"]
        same_l = ra is not None and rb is not None and ra["launches"] == rb["launches"]
        bad += not (same_h and same_l)
        n = len(ra["hashes"]) if ra else 0
        print(f"{key:32s} {n} outputs: hashes {'equal' if same_h else 'DIFFER'}; "
              f"{len(ra['launches']) if ra else 0} launches: {'equal' if same_l else 'DIFFER'}")
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--host-cost", action="store_true")
    ap.add_argument("--compare", nargs=2, default=None)
    a = ap.parse_args()
    if a.compare:
        return compare(*a.compare)
    if a.host_cost:
        return host_cost()
    return record(a.out or "ab_module_bits.json")


if __name__ == "__main__":
    sys.exit(main())
