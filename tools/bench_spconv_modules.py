"""Dev tool: FPNSpMiddleResNetFHD's graph rebuilt from al3d.spconv modules against the built-in encoder, and the three layer
types only the modules have, on the synthetic pool's rulebooks.

  python tools/bench_spconv_modules.py [batch=8] [reps=5]

Part 1 times the whole sparse stage both ways on one batch (index work included in both: the built-in encoder's
build_rulebook + run, the modules' per-layer site / table builds), from the same weights, and prints the largest
difference of the two BEV maps relative to the map's largest value.  The module graph is written the way the reference's
scn.py writes it: SparseSequential stages (their conv -> BatchNorm1d -> ReLU runs fold into one launch) and residual blocks
that call their BatchNorm and the residual add on ``.features`` (unfused, as any user's block does).

Part 2 times SparseMaxPool3d, SparseInverseConv3d and SparseConvTranspose3d at each level's size (the input rows of the
level's strided conv and the geometry of that conv), a fresh tensor per call ("cold": check + sites + table + launch) and with
the rulebook found under its indice_key ("warm": the launch alone; the pool has no key), next to the bytes the launch
fetches (table entries, gathered rows, weights) and writes (output rows)."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from torch import nn

import al3d.spconv as spconv
from al3d import synthetic
from al3d.datasets import DeviceSweepLoader, PoolFrames, generate_task_anchors
from al3d.models import build_detector
from al3d.utils import Config

dev = torch.device("cuda:0")
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
bs = int(sys.argv[1]) if len(sys.argv) > 1 else 8
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5


def bn(c):
    return nn.BatchNorm1d(c, eps=1e-3, momentum=0.01)


class Block(spconv.SparseModule):
    """scn.py's SparseBasicBlock on the module API."""

    def __init__(self, c, key):
        super().__init__()
        self.conv1 = spconv.SubMConv3d(c, c, 3, bias=True, indice_key=key)
        self.bn1 = bn(c)
        self.relu = nn.ReLU()
        self.conv2 = spconv.SubMConv3d(c, c, 3, bias=True, indice_key=key)
        self.bn2 = bn(c)

    def forward(self, x):
        identity = x.features
        out = self.conv1(x)
        out.features = self.relu(self.bn1(out.features))
        out = self.conv2(out)
        out.features = self.relu(self.bn2(out.features) + identity)
        return out


class ModuleEncoder(nn.Module):
    """Same child names as the built-in FPNSpMiddleResNetFHD: its state dict loads strictly."""

    def __init__(self, cin):
        super().__init__()
        S, C, Sub = spconv.SparseSequential, spconv.SparseConv3d, spconv.SubMConv3d
        self.middle_conv0 = S(Sub(cin, 16, 3, bias=False, indice_key="res0"), bn(16), nn.ReLU(), Block(16, "res0"),
                              Block(16, "res0"), C(16, 32, 3, 2, padding=1, bias=False, indice_key="d0"), bn(32), nn.ReLU())
        self.middle_conv1 = S(Block(32, "res1"), Block(32, "res1"),
                              C(32, 64, 3, 2, padding=1, bias=False, indice_key="d1"), bn(64), nn.ReLU())
        self.middle_conv2 = S(Block(64, "res2"), Block(64, "res2"),
                              C(64, 128, 3, 2, padding=[0, 1, 1], bias=False, indice_key="d2"), bn(128), nn.ReLU())
        self.middle_conv3 = S(Block(128, "res3"), Block(128, "res3"),
                              C(128, 128, (3, 1, 1), (2, 1, 1), bias=False, indice_key="d3"), bn(128), nn.ReLU())

    def stages(self):
        return [self.middle_conv0, self.middle_conv1, self.middle_conv2, self.middle_conv3]

    def forward(self, feats, coords, batch, shape):
        x = spconv.SparseConvTensor(feats, coords, shape, batch)
        levels = []
        for st in self.stages():
            levels.append(x)
            x = st(x)
        B, C, Dz, H, W = (batch, x.features.shape[1], *x.spatial_shape)
        return x.dense().view(B, C * Dz, H, W), levels


def timed(fn, n=reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def launch_bytes(tab, cin, cout, wbytes):
    nbr = tab["nbr"]
    valid = int((nbr >= 0).sum())
    return nbr.numel() * 4 + valid * cin * 4 + wbytes, tab["n"] * cout * 4


def main():
    cfg = Config.fromfile(os.path.join(root, "examples/active/cbgs_spatial_temporal_feature.py"))
    model = build_detector(cfg.model, train_cfg=None, test_cfg=cfg.test_cfg)
    synthetic.seeded_init_(model, seed=0)
    model = model.to(dev).eval()
    anchors = generate_task_anchors(cfg.tasks, cfg.target_assigner.anchor_generators, [1, 128, 128])
    pool = PoolFrames.from_synthetic(bs, dev, num_base=8)
    ex = next(iter(DeviceSweepLoader(pool, cfg.voxel_generator, anchors, batch_size=bs, device=dev)))
    feats, coords = ex["voxel_features"], ex["coordinates"]
    shape = [int(v) for v in (np.array(ex["shape"][0][::-1]) + [1, 0, 0])]
    enc = model.backbone
    mods = ModuleEncoder(feats.shape[1])
    mods.load_state_dict(enc.state_dict(), strict=True)
    mods = mods.to(dev).eval()

    with torch.no_grad():
        ref, _ = enc(feats, coords, bs, ex["shape"][0])                     # [B, H, W, C*D]
        got, levels = mods(feats, coords, bs, shape)                        # [B, C*D, H, W]
        diff = float((got.permute(0, 2, 3, 1) - ref).abs().max() / ref.abs().max())
        t_enc = timed(lambda: enc(feats, coords, bs, ex["shape"][0]))
        t_mod = timed(lambda: mods(feats, coords, bs, shape))
    print(f"batch {bs}, {feats.shape[0]} voxels: built-in encoder {t_enc:.2f} ms, module graph {t_mod:.2f} ms, ratio "
          f"{t_mod / t_enc:.2f}; max |module - built-in| / max |built-in| = {diff:.2e}")

    print("layer            level rows_in rows_out  C   cold ms  warm ms   fetched MB  written MB")
    downs = [st[-3] for st in mods.stages()]
    for li, (x, down, st) in enumerate(zip(levels, downs, mods.stages())):
        with torch.no_grad():
            x = spconv.SparseSequential(*list(st.children())[:-3])(x)       # the rows the level's strided conv reads
        k, s, p = down.kernel_size, down.stride, down.padding
        n, c = x.features.shape[0], x.features.shape[1]
        co = down.out_channels

        def fresh(f=x.features):
            return spconv.SparseConvTensor(f, x.indices, x.spatial_shape, bs)
        with torch.no_grad():
            pool_ = spconv.SparseMaxPool3d(k, s, p)
            out = pool_(fresh())
            from al3d import detector_ops as D
            tab = D.sparse_table(False, out.indices, out.indices.shape[0], bs, x.spatial_shape, x.index_grid(), k, s, p)
            fb, wb = launch_bytes(tab, c, c, 0)
            print(f"SparseMaxPool3d      {li}  {n:7d} {out.indices.shape[0]:7d} {c:3d} {timed(lambda: pool_(fresh())):8.3f}        -"
                  f"   {fb / 1e6:9.2f}  {wb / 1e6:9.2f}")
            # inverse: the level's strided conv stores the key, the inverse layer maps its output rows back
            mid = down(fresh())
            inv = spconv.SparseInverseConv3d(co, co, k, indice_key=down.indice_key).to(dev)
            back = inv(mid)
            book = mid.find_indice_pair(down.indice_key)[2].inverse
            fb, wb = launch_bytes(next(iter(book.tables.values())), co, co, inv.weight.numel() * 4)

            def cold_inv():
                m_ = down(fresh())
                return inv(m_)
            t_pair = timed(cold_inv) - timed(lambda: down(fresh()))
            print(f"SparseInverseConv3d  {li}  {mid.indices.shape[0]:7d} {back.indices.shape[0]:7d} {co:3d} {t_pair:8.3f} "
                  f"{timed(lambda: inv(mid)):8.3f}   {fb / 1e6:9.2f}  {wb / 1e6:9.2f}")
            # transposed: the same geometry upwards from the next level's rows
            up = spconv.SparseConvTranspose3d(co, co, k, s, p, indice_key="up").to(dev)

            def fresh_mid():
                return spconv.SparseConvTensor(mid.features, mid.indices, mid.spatial_shape, bs)
            keyed = fresh_mid()
            o = up(keyed)
            fb, wb = launch_bytes(next(iter(keyed.find_indice_pair("up")[2].tables.values())), co, co, up.weight.numel() * 4)
            print(f"SparseConvTranspose3d {li} {mid.indices.shape[0]:7d} {o.indices.shape[0]:7d} {co:3d} "
                  f"{timed(lambda: up(fresh_mid())):8.3f} {timed(lambda: up(keyed)):8.3f}   {fb / 1e6:9.2f}  {wb / 1e6:9.2f}")


if __name__ == "__main__":
    main()
