"""CenterPoint's CenterHead, inference half (the head of the reference's ``det/centerhead/**`` configs).

Reference: bevfusion/mmdet3d/models/heads/bbox/centerpoint.py:20-125 (``SeparateHead``), :249-366 (``CenterHead``
construction and ``forward_single``), :637-884 (``get_bboxes``, ``get_task_detections``); coder
core/bbox/coders/centerpoint_bbox_coders.py; settings configs/nuscenes/det/centerhead/default.yaml.  Training (targets,
losses) is out of scope: the sweep runs ``eval()`` only.

What runs where: ``shared_conv`` (3x3, in -> 64, BN, ReLU) and the first layers of the separate heads (3x3, 64 -> 64, BN,
ReLU; all heads of a task as ONE dense launch with Cout = 64 x heads) go through this build's dense conv kernels under
``AL3D_MATH``; the last layers of a task (3x3, 64 -> 1..3 channels, bias) are one ``al3d_conv3x3_grouped_nhwc_f32``
launch that writes straight into the head's channels-last output ``[B, H, W, sum of all heads' channels]``; the whole
post-processing is ``al3d_center_decode_nms_f32`` on that buffer.  The 64-channel intermediates of a task are
``H * W * 64 * heads * 4`` bytes per sample (50 MB at 180 x 180 with six heads), so a batch runs task by task and in
frame chunks of at most ``CHUNK_BYTES`` ("CenterHead").

Parameter names follow the reference module tree (mmcv's ``ConvModule`` gives ``<name>.conv`` / ``<name>.bn``), so its
state dicts load strictly.
"""
import copy

import torch
from torch import nn

from .. import detector_ops as D
from ..weight_cache import PackCache
from .conv_layers import FoldedConv
from .registry import HEADS


class _ConvModule2d(nn.Module):
    """mmcv ``ConvModule`` with a norm layer: conv (no bias) -> bn -> ReLU, parameter container only."""

    def __init__(self, cin, cout, k):
        super().__init__()
        self.conv = nn.Conv2d(cin, cout, k, padding=k // 2, bias=False)
        self.bn = nn.BatchNorm2d(cout)


@HEADS.register_module
class SeparateHead(nn.Module):
    """centerpoint.py:20-125: per regression target ``ConvModule(in -> head_conv)`` x (num_conv - 1) +
    ``Conv2d(head_conv -> classes, bias)``.  The device path is built for what every CenterHead config uses: two layers
    per target, 3 x 3 kernels, 64 channels in between, at most 8 output channels per target."""

    CHUNK_BYTES = 128 << 20

    def __init__(self, in_channels, heads, head_conv=64, final_kernel=1, init_bias=-2.19, conv_cfg=None, norm_cfg=None,
                 bias="auto", init_cfg=None, transpose_input=False, **_unused):
        super().__init__()
        assert init_cfg is None, "To prevent abnormal initialization behavior, init_cfg is not allowed to be set"
        self.heads, self.init_bias, self.transpose_input = dict(heads), init_bias, bool(transpose_input)
        self.in_channels, self.head_conv, self.final_kernel = in_channels, head_conv, final_kernel
        for head, (classes, num_conv) in self.heads.items():
            layers, c_in = [], in_channels
            for _ in range(num_conv - 1):
                layers.append(_ConvModule2d(c_in, head_conv, final_kernel))
                c_in = head_conv
            layers.append(nn.Conv2d(c_in, classes, final_kernel, padding=final_kernel // 2, bias=True))
            setattr(self, head, nn.Sequential(*layers))
        if "heatmap" in self.heads:
            getattr(self, "heatmap")[-1].bias.data.fill_(init_bias)
        # all targets' first layers as ONE dense launch, their 64 channels side by side (other depths: _check refuses them)
        if all(n == 2 for _, n in self.heads.values()):
            self._first = FoldedConv([(getattr(self, h)[0].conv, getattr(self, h)[0].bn) for h in self.heads],
                                     swap_hw=self.transpose_input)
        self._last = PackCache()

    @property
    def out_channels(self):
        return sum(c for c, _ in self.heads.values())

    def spans(self, base=0):
        """{target: (first channel, end)} inside the task's window of the fused output, targets in ``heads`` order."""
        out, o = {}, base
        for h, (c, _) in self.heads.items():
            out[h] = (o, o + c)
            o += c
        return out

    def _check(self):
        if self.final_kernel != 3 or self.head_conv != 64 or any(n != 2 for _, n in self.heads.values()) or \
                any(c > 8 for c, _ in self.heads.values()):
            raise NotImplementedError("SeparateHead's kernels are built for num_conv = 2, final_kernel = 3, head_conv = 64 "
                                      "and <= 8 channels per target (every CenterHead config of the reference)")

    def pack(self, device):
        """(grouped weights [sum of channels, 9, 64], bias) of the targets' last layers."""
        self._check()
        last = [getattr(self, h)[1] for h in self.heads]

        def build():
            ws = [m.weight.detach().float() for m in last]
            w2 = torch.cat([D.pack_conv_weight(w.transpose(2, 3) if self.transpose_input else w) for w in ws])
            return w2.to(device).contiguous(), torch.cat([m.bias.detach().float() for m in last]).to(device).contiguous()
        return self._last.get(device, last, None, build)             # an fp32 kernel: one variant

    def run_into(self, x, out, base):
        """x [B,H,W,in] channels-last -> this task's channels written at ``base`` of ``out`` [B,H,W,CH]."""
        w2, b2 = self.pack(x.device)
        B, H, W, _ = x.shape
        G = len(self.heads)
        cout = [c for c, _ in self.heads.values()]
        coff = [a for a, _ in self.spans(base).values()]
        n = max(1, self.CHUNK_BYTES // (H * W * G * 64 * 4))
        for s in range(0, B, n):
            D.conv3x3_grouped_nhwc(self._first(x[s:s + n]), w2, b2, cout, coff, out=out[s:s + n])
        return out

    def forward(self, x):
        """x channels-last [B,H,W,in] -> {target: [B, classes, H, W]} (views of one channels-last buffer)."""
        if self.training:
            raise RuntimeError("al3d SeparateHead implements the eval() path only")
        B, H, W, _ = x.shape
        out = torch.empty((B, H, W, self.out_channels), dtype=torch.float32, device=x.device)
        self.run_into(x, out, 0)
        return {h: out[..., a:b].permute(0, 3, 1, 2) for h, (a, b) in self.spans().items()}


class CenterPreds(list):
    """``forward``'s result: the reference's structure (per task ``[dict(target -> [B, C, H, W])]``) whose tensors are
    views of ``fused`` [B,H,W,CH], the buffer the post-processing kernel reads."""
    fused = None


@HEADS.register_module
class CenterHead(nn.Module):
    """Inference restatement of the reference head.  ``forward(x)``: x channels-last BEV map [B,H,W,in_channels] ->
    per task ``[dict]`` with the reference's keys (reg, height, dim, rot, vel, heatmap: [B,C,H,W]);
    ``get_bboxes(preds)`` -> per sample dict(bboxes [K,9|7], scores, labels), tasks merged as centerpoint.py:738-757.

    The reference's maps are [x, y]; this build's detector maps are [H = y, W = x].  With ``transpose_input`` the head
    keeps the reference's meaning behind this build's necks WITHOUT transposing the map: the 3 x 3 kernels are packed
    with their spatial axes swapped and the decode reads x from the W index and y from the H index.  The maps in
    ``forward``'s dicts are then [B,C,y,x]."""

    def __init__(self, in_channels=(128,), tasks=None, train_cfg=None, test_cfg=None, bbox_coder=None, common_heads=None,
                 loss_cls=None, loss_bbox=None, separate_head=None, share_conv_channel=64, num_heatmap_convs=2,
                 conv_cfg=None, norm_cfg=None, bias="auto", norm_bbox=True, init_cfg=None, transpose_input=False, **_unused):
        super().__init__()
        assert init_cfg is None, "To prevent abnormal initialization behavior, init_cfg is not allowed to be set"
        tasks = [t["class_names"] if isinstance(t, dict) else t for t in (tasks or [])]
        self.class_names = [list(t) for t in tasks]                   # grouped by task (read by PPALSelector)
        self.num_classes = [len(t) for t in tasks]
        self.train_cfg, self.test_cfg, self.bbox_coder = train_cfg, dict(test_cfg or {}), dict(bbox_coder or {})
        if isinstance(in_channels, (list, tuple)):
            in_channels = in_channels[0]
        self.in_channels, self.norm_bbox, self.transpose_input = in_channels, norm_bbox, bool(transpose_input)
        self.shared_conv = _ConvModule2d(in_channels, share_conv_channel, 3)
        sep = dict(separate_head or dict(type="SeparateHead", init_bias=-2.19, final_kernel=3))
        kind = sep.pop("type", "SeparateHead")
        if kind != "SeparateHead":
            raise NotImplementedError(f"separate_head type {kind!r}: only SeparateHead is built (DCNSeparateHead needs deformable convolutions)")
        self.task_heads = nn.ModuleList()
        for num_cls in self.num_classes:
            heads = copy.deepcopy(dict(common_heads or {}))
            heads.update(dict(heatmap=(num_cls, num_heatmap_convs)))
            self.task_heads.append(SeparateHead(in_channels=share_conv_channel, heads=heads, transpose_input=self.transpose_input,
                                                **{k: v for k, v in sep.items() if k not in ("in_channels", "heads", "num_cls")}))
        self._shared = FoldedConv([(self.shared_conv.conv, self.shared_conv.bn)], swap_hw=self.transpose_input)

    # ---------------------------------------------------------------- graph
    def _layout(self):
        """(channels of the fused output, per task {target: (start, end)})."""
        spans, base = [], 0
        for th in self.task_heads:
            spans.append(th.spans(base))
            base += th.out_channels
        return base, spans

    def forward(self, x, finetune=False, **_unused):
        if self.training:
            raise RuntimeError("al3d CenterHead implements the eval() path only")
        feat = self._shared(x)
        B, H, W, _ = feat.shape
        CH, spans = self._layout()
        fused = torch.empty((B, H, W, CH), dtype=torch.float32, device=x.device)
        preds = CenterPreds()
        for th, sp in zip(self.task_heads, spans):
            th.run_into(feat, fused, min(a for a, _ in sp.values()))
            preds.append([{h: fused[..., a:b].permute(0, 3, 1, 2) for h, (a, b) in sp.items()}])
        preds.fused = fused
        return preds

    # ---------------------------------------------------------------- post-processing
    def _nms_scales(self):
        cfg = self.test_cfg                                            # centerpoint.py:651-666
        if "nms_scale" in cfg:
            if not isinstance(cfg["nms_scale"], (list, tuple)):
                return [[cfg["nms_scale"]] * n for n in self.num_classes]
            return cfg["nms_scale"]
        return [[1.0] * n for n in self.num_classes]

    @staticmethod
    def _read_counts(counts):
        """The one host read of the post-processing: detections per (sample, task)."""
        return counts.cpu().tolist()

    def get_bboxes(self, preds_dicts, metas=None, **_unused):
        """centerpoint.py:637-757 as one device call plus one read of the counts."""
        fused = getattr(preds_dicts, "fused", None)
        _, spans = self._layout()
        if fused is None:                                              # hand-made predictions: assemble the buffer
            fused = torch.cat([p[0][h] for p, sp in zip(preds_dicts, spans) for h in sp], dim=1).permute(0, 2, 3, 1).contiguous()
        chan = [[sp[h][0] if h in sp else -1 for h in D.CENTER_CHANNELS] for sp in spans]
        for sp in spans:
            missing = [h for h in ("heatmap", "height", "dim", "rot") if h not in sp]
            if missing:
                raise KeyError(f"CenterHead: common_heads lacks {missing}")
        c, t = self.bbox_coder, self.test_cfg
        if t.get("max_pool_nms"):
            raise NotImplementedError("max_pool_nms is not built (every centerhead config of the reference sets it false)")
        boxes, scores, labels, counts = D.center_decode_nms(
            fused, self.num_classes, chan, swapped=self.transpose_input, max_num=c.get("max_num", 100),
            norm_bbox=self.norm_bbox, out_size_factor=c["out_size_factor"], voxel_size=c["voxel_size"], pc_range=c["pc_range"],
            coder_score_threshold=c.get("score_threshold"), post_center_range=c["post_center_range"],
            nms_type=t["nms_type"], nms_scale=self._nms_scales(), min_radius=t.get("min_radius", [0.0] * len(spans)),
            score_threshold=t.get("score_threshold", 0.0), nms_thr=t.get("nms_thr", 0.0),
            pre_max_size=t.get("pre_max_size", 1 << 30) or (1 << 30), post_max_size=t["post_max_size"],
            post_center_limit_range=t.get("post_center_limit_range"), merge=True)
        width = 9 if all("vel" in sp for sp in spans) else 7
        host = self._read_counts(counts)
        rets = []
        for b, row in enumerate(host):
            rets.append(dict(bboxes=torch.cat([boxes[b, k, :n, :width] for k, n in enumerate(row)]),
                             scores=torch.cat([scores[b, k, :n] for k, n in enumerate(row)]),
                             labels=torch.cat([labels[b, k, :n] for k, n in enumerate(row)]).long()))
        return rets

    def predict(self, example, preds_dicts, test_cfg=None, **_unused):
        """The det3d head contract (``bbox_head.predict(example, preds, test_cfg)``, voxelnet.py:73-81) over
        ``get_bboxes``.  ``test_cfg`` is the DETECTOR's (det3d anchor-head settings) and is not read: like the reference
        head, CenterHead post-processes by the ``test_cfg`` it was built with.  One dict per sample with ``box3d_lidar`` [K, 9|7], ``scores``, ``label_preds``, ``metadata`` --
        what the uncertainty selectors read (det3d/selectors/entropy_selector.py:50-86: ``output['scores']``)."""
        rets = self.get_bboxes(preds_dicts)
        metas = (example.get("metadata", None) if isinstance(example, dict) else None) or [None] * len(rets)
        return [dict(box3d_lidar=r["bboxes"], scores=r["scores"], label_preds=r["labels"], metadata=m)
                for r, m in zip(rets, metas)]
