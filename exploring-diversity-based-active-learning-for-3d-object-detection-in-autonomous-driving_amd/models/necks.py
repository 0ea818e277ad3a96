"""SECOND-style dense neck (reference det3d/models/necks/rpn.py:22-159).

Same module tree / parameter names as the reference (``blocks.<b>.<i>``, ``deblocks.<b>.<i>``)
so its state dicts load; the forward pass runs the fused conv+BN+ReLU MFMA kernels on
NHWC activations and writes both deblock outputs straight into the concatenated
``[B,128,128,512]`` buffer (no ``torch.cat`` copy).
"""
import numpy as np
import torch
from torch import nn

from .. import detector_ops as D
from ..weight_cache import PackCache
from .registry import NECKS


@NECKS.register_module
class RPN(nn.Module):
    def __init__(self, layer_nums, ds_layer_strides, ds_num_filters, us_layer_strides,
                 us_num_filters, num_input_features, norm_cfg=None, name="rpn", logger=None,
                 **kwargs):
        super().__init__()
        self._layer_strides = ds_layer_strides
        self._num_filters = ds_num_filters
        self._layer_nums = layer_nums
        self._upsample_strides = us_layer_strides
        self._num_upsample_filters = us_num_filters
        self._num_input_features = num_input_features
        assert len(ds_layer_strides) == len(layer_nums) == len(ds_num_filters)
        assert len(us_num_filters) == len(us_layer_strides)
        self._upsample_start_idx = len(layer_nums) - len(us_layer_strides)
        eps = 1e-3 if norm_cfg is None else norm_cfg.get("eps", 1e-5)
        mom = 0.01 if norm_cfg is None else norm_cfg.get("momentum", 0.1)

        def bn(c):
            return nn.BatchNorm2d(c, eps=eps, momentum=mom)

        in_filters = [num_input_features, *ds_num_filters[:-1]]
        blocks, deblocks = [], []
        for i, layer_num in enumerate(layer_nums):
            planes = ds_num_filters[i]
            layers = [nn.ZeroPad2d(1), nn.Conv2d(in_filters[i], planes, 3, stride=ds_layer_strides[i], bias=False),
                      bn(planes), nn.ReLU()]
            for _ in range(layer_num):
                layers += [nn.Conv2d(planes, planes, 3, padding=1, bias=False), bn(planes), nn.ReLU()]
            blocks.append(nn.Sequential(*layers))
            if i - self._upsample_start_idx >= 0:
                stride = us_layer_strides[i - self._upsample_start_idx]
                cout = us_num_filters[i - self._upsample_start_idx]
                if stride > 1:
                    up = nn.ConvTranspose2d(planes, cout, stride, stride=stride, bias=False)
                else:
                    s = int(np.round(1 / stride))
                    up = nn.Conv2d(planes, cout, s, stride=s, bias=False)
                deblocks.append(nn.Sequential(up, bn(cout), nn.ReLU()))
        self.blocks = nn.ModuleList(blocks)
        self.deblocks = nn.ModuleList(deblocks)
        self.packs = PackCache()
        if logger is not None:
            logger.info("Finish RPN Initialization")

    @property
    def downsample_factor(self):
        factor = np.prod(self._layer_strides)
        if len(self._upsample_strides) > 0:
            factor /= self._upsample_strides[-1]
        return factor

    def init_weights(self):
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.xavier_uniform_(m.weight)

    def _prepare(self, device):
        """Fold and pack every layer for the dense dispatch: once per arithmetic / structure (a sweep that re-runs a batch
        under bf16x6, AL3D_MATH=auto, flips back without re-packing) and again after a parameter or buffer is written."""
        def layer(conv, bn, *geom, deconv=False):
            w, scale, shift = D.fold_conv_bn([(conv, bn)], deconv=deconv)
            w, scale = D.pack_dense(w.to(device), scale.to(device), *geom)
            return dict(w=w, scale=scale, shift=shift.to(device))

        def build():
            blocks, deblocks = [], []
            for blk in self.blocks:
                mods = list(blk.children())
                convs = []
                for j, m in enumerate(mods):
                    if isinstance(m, nn.Conv2d):
                        pad = 1 if (j > 0 and isinstance(mods[j - 1], nn.ZeroPad2d)) else m.padding[0]
                        convs.append(dict(layer(m, mods[j + 1], m.kernel_size[0], m.stride[0], pad),
                                          k=m.kernel_size[0], s=m.stride[0], p=pad))
                blocks.append(convs)
            for up, bn, _ in self.deblocks:
                if isinstance(up, nn.ConvTranspose2d):
                    assert up.kernel_size == (2, 2) and up.stride == (2, 2), "only 2x2/s2 deconv is built"
                    deblocks.append(dict(layer(up, bn, "deconv", deconv=True), deconv=True))
                else:
                    deblocks.append(dict(layer(up, bn, up.kernel_size[0], up.stride[0], 0), deconv=False,
                                         k=up.kernel_size[0], s=up.stride[0]))
            return blocks, deblocks
        layers = [m for seq in (*self.blocks, *self.deblocks) for m in seq]
        self._blocks_p, self._deblocks_p = self.packs.get(device, layers, (D.MATH, D.DENSE), build)

    def _kind(self, w):
        return getattr(w, "kind", None)

    def rows_input_ok(self):
        """Can ``forward`` take the sparse encoder's last level as ``detector_ops.BevRows`` (two z levels) right now?
        It needs the first conv on the streamed 3x3 f16x3 kernel; decided from the module, before any packing."""
        conv = next((m for m in self.blocks[0] if isinstance(m, nn.Conv2d)), None)
        if conv is None or conv.in_channels % 2:
            return False
        kind = D.dense_structure(conv.out_channels, conv.in_channels, conv.kernel_size[0], conv.stride[0], 1)
        return D.neck_rows_ok(kind, 2, conv.in_channels // 2)

    def forward(self, x, out_pair=False):
        """x NHWC [B,H,W,Cin] (or the encoder's ``detector_ops.BevRows``: the first conv then reads the sparse rows)
        -> NHWC [B,H',W',sum(us_num_filters)].

        Pair pixels (csrc/sp_rows.h, ``AL3D_DPIX``): a block's output whose consumers all run on the LDS-DMA kernel (the
        next block's strided entry conv, the block's deblock) is written as pair pixels by the block's last 3x3 launch
        and read without a split -- invisible outside.  ``out_pair=True`` asks for the concatenated map in that format
        too (for a head on the LDS-DMA kernel); ``self.last_out_pair`` says whether it was granted (it needs the fused
        GAP: the embedding is then taken from the f32 values inside the deblock launches)."""
        if self.training:
            raise RuntimeError("al3d RPN implements the eval() sweep only")
        self._prepare(x.device)
        if isinstance(x, D.BevRows) and not D.neck_rows_ok(self._kind(self._blocks_p[0][0]["w"]), x.index.shape[3],
                                                           x.rows.shape[1]):
            x = x.dense()                                 # the first conv has no rows input under this arithmetic / structure
        pairing = D.MATH == "f16x3" and D.DPIX == "pair"
        out, coff = None, 0
        ctot = sum(self._num_upsample_filters)
        # fused GAP: every deblock launch runs on the generic f16x3 kernel (plain planes) -> they can emit the
        # embedding's partial sums while they store the map (saves re-reading 33.5 MB per frame)
        fuse = D.GAP == "fused" and len(self._deblocks_p) == len(self._blocks_p) - self._upsample_start_idx and             all(D.gap_fusable(d["w"]) for d in self._deblocks_p)
        gap, self.embedding = None, None
        out_pair = bool(out_pair and pairing and fuse and all(self._kind(d["w"]) == "dma" for d in self._deblocks_p))
        self.last_out_pair = out_pair
        x_pair = False
        for i, convs in enumerate(self._blocks_p):
            j = i - self._upsample_start_idx
            # may this block's output be pair pixels?  every consumer must be an LDS-DMA launch
            consumers = []
            if j >= 0:
                consumers.append(self._deblocks_p[j]["w"])
            if i + 1 < len(self._blocks_p):
                consumers.append(self._blocks_p[i + 1][0]["w"])
            blk_pair = pairing and len(convs) > 1 and self._kind(convs[-1]["w"]) in ("frag3x3", "wino") and \
                convs[-1]["scale"].shape[0] % 8 == 0 and all(self._kind(w) == "dma" for w in consumers)
            for ci, c in enumerate(convs):
                io = 0
                if ci == 0 and x_pair:
                    io |= D.IO_IN_PAIR
                if ci == len(convs) - 1 and blk_pair:
                    io |= D.IO_OUT_PAIR
                assert ci == 0 or not (io & D.IO_IN_PAIR)
                x = D.conv2d_nhwc(x, c["w"], c["scale"], c["shift"], c["k"], c["s"], c["p"], True, io=io)
            x_pair = blk_pair
            if j >= 0:
                d = self._deblocks_p[j]
                B, H, W, _ = x.shape
                if d["deconv"]:
                    oh, ow = 2 * H, 2 * W
                else:
                    oh = (H - d["k"]) // d["s"] + 1
                    ow = (W - d["k"]) // d["s"] + 1
                if out is None:
                    out = torch.empty((B, oh, ow, ctot), dtype=torch.float32, device=x.device)
                g = None
                if fuse:
                    if tuple(out.shape[1:3]) != (oh, ow):
                        fuse, gap = False, None                     # deblocks of different output sizes: stand-alone GAP
                    else:
                        if gap is None:
                            # one buffer for all deblocks; launches with fewer workgroup partials leave zeros behind
                            all_parts = [D.gap_parts(oh, ow, dd["deconv"]) for dd in self._deblocks_p]
                            gap = (torch.zeros if len(set(all_parts)) > 1 else torch.empty)(
                                (B, max(all_parts), ctot), dtype=torch.float32, device=x.device)
                        g = gap
                dio = (D.IO_IN_PAIR if x_pair else 0) | (D.IO_OUT_PAIR if out_pair else 0)
                if d["deconv"]:
                    D.deconv2x2_nhwc(x, d["w"], d["scale"], d["shift"], True, out=out, coff=coff, gap=g, io=dio)
                else:
                    D.conv2d_nhwc(x, d["w"], d["scale"], d["shift"], d["k"], d["s"], 0, True, out=out,
                                  coff=coff, gap=g, io=dio)
                coff += d["scale"].shape[0]
        if fuse and gap is not None and out is not None and coff == ctot:
            self.embedding = D.gap_reduce_parts(gap, out.shape[1] * out.shape[2])
        if out_pair and self.embedding is None:          # the fused GAP was dropped on the way: hand out f32 after all
            out = D.rows_convert(out.view(-1, ctot), False).view_as(out)
            self.last_out_pair = False
        assert out is not None or not x_pair
        return out if out is not None else x
