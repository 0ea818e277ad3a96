"""Sparse 3-D ResNet middle encoder (reference det3d/models/backbones/scn.py:54-97,316-392).

Module tree and parameter names/layouts match the reference + spconv 1.2.1 so its
checkpoints load: ``middle_conv{0..3}.<i>.weight [kz,ky,kx,Cin,Cout]``, SparseBasicBlock
``conv{1,2}.{weight,bias}`` / ``bn{1,2}.*``.  The forward pass is a list of fused HIP layers
(csrc/spconv.hip): conv + bias + BN(eval) (+residual) (+ReLU) per launch.
"""
import numpy as np
import torch
from torch import nn

from .. import lib
from .. import detector_ops as D
from ..detector_ops import fold_bn
from ..selector_ops import _ptr, _stream
from ..weight_cache import PackCache
from .registry import BACKBONES


class _SpConvParams(nn.Module):
    """Parameter holder with spconv's layout ``weight [*k, Cin, Cout]``."""

    def __init__(self, cin, cout, ksize, stride=1, padding=0, bias=False, subm=False):
        super().__init__()
        k = tuple(ksize) if isinstance(ksize, (tuple, list)) else (ksize,) * 3
        s = tuple(stride) if isinstance(stride, (tuple, list)) else (stride,) * 3
        p = tuple(padding) if isinstance(padding, (tuple, list)) else (padding,) * 3
        self.in_channels, self.out_channels = cin, cout
        self.kernel_size, self.stride, self.padding, self.subm = k, s, p, subm
        self.weight = nn.Parameter(torch.empty(*k, cin, cout))
        if bias:
            self.bias = nn.Parameter(torch.zeros(cout))
        else:
            self.register_parameter("bias", None)
        fan = cin * int(np.prod(k))
        nn.init.uniform_(self.weight, -1.0 / fan ** 0.5, 1.0 / fan ** 0.5)


class SubMConv3d(_SpConvParams):
    def __init__(self, cin, cout, ksize, bias=True, indice_key=None):
        super().__init__(cin, cout, ksize, 1, 0, bias, subm=True)
        self.indice_key = indice_key


class SparseConv3d(_SpConvParams):
    def __init__(self, cin, cout, ksize, stride=1, padding=0, bias=True):
        super().__init__(cin, cout, ksize, stride, padding, bias, subm=False)


class SparseBasicBlock(nn.Module):
    """conv1-bn1-relu-conv2-bn2-(+identity)-relu; the convs carry a bias (scn.py:68-73)."""

    def __init__(self, inplanes, planes, indice_key=None):
        super().__init__()
        self.conv1 = SubMConv3d(inplanes, planes, 3, bias=True, indice_key=indice_key)
        self.bn1 = nn.BatchNorm1d(planes, eps=1e-3, momentum=0.01)
        self.relu = nn.ReLU()
        self.conv2 = SubMConv3d(planes, planes, 3, bias=True, indice_key=indice_key)
        self.bn2 = nn.BatchNorm1d(planes, eps=1e-3, momentum=0.01)


class SparseTensor:
    """Minimal stand-in for spconv.SparseConvTensor: features [N,C] f32, indices [N,4] i32."""

    def __init__(self, features, indices, spatial_shape, batch_size, pair_rows=False):
        # pair_rows: ``features`` is in the f16x3 kernels' pair-row format (csrc/sp_rows.h); converted on first access
        self._features, self._pair = features, pair_rows
        self.indices = indices
        self.spatial_shape, self.batch_size = list(spatial_shape), batch_size

    @property
    def features(self):
        if self._pair:
            self._features, self._pair = D.rows_convert(self._features, to_pair=False), False
        return self._features


def _bn(c):
    return nn.BatchNorm1d(c, eps=1e-3, momentum=0.01)


class _Level:
    """Dense index grid of one resolution level, kept in HBM across calls."""

    def __init__(self, shape, max_batch, device):
        self.D, self.H, self.W = [int(s) for s in shape]
        self.max_batch = max_batch
        self.grid = torch.full((max_batch * self.D * self.H * self.W,), -1, dtype=torch.int32,
                               device=device)


class _SparseEncoderBase(nn.Module):
    def __init__(self):
        super().__init__()
        self.packs = PackCache()

    def _stages(self):
        raise NotImplementedError

    def _prepare(self, device):
        """Choose every layer's structure (detector_ops.sparse_structure), then pack weights / fold BN once per device
        and structure list (eval only)."""
        # The input level's rows may be renumbered (raster order, csrc/spconv_l0.hip) only if they never leave the encoder:
        # a strided conv must come before the first stage output (true for every shipped encoder; a stage that ends on the
        # input level keeps the caller's row order, like spconv's SubMConv3d)
        first = list(self._stages()[0].children()) if len(self._stages()) else []
        raster_ok = any(isinstance(m_, _SpConvParams) and not m_.subm for m_ in first)
        plan = []
        for seq in self._stages():
            mods = list(seq.children())
            i = 0
            while i < len(mods):
                m = mods[i]
                if isinstance(m, _SpConvParams):
                    plan.append(dict(kind="subm" if m.subm else "down", mod=m, bn=mods[i + 1], residual=False))
                    i += 3  # conv, bn, relu
                elif isinstance(m, SparseBasicBlock):
                    plan.append(dict(kind="subm", mod=m.conv1, bn=m.bn1, bias=True, residual=False, block_start=True))
                    plan.append(dict(kind="subm", mod=m.conv2, bn=m.bn2, bias=True, residual=True))
                    i += 1
                else:
                    i += 1
            plan.append(dict(kind="stage_end"))
        convs = [s_ for s_ in plan if s_["kind"] != "stage_end"]
        for s_ in convs:
            m = s_["mod"]
            s_["sp"], s_["cin"], s_["cols"] = D.sparse_structure(m.in_channels, m.out_channels, int(np.prod(m.kernel_size)),
                                                                 m.subm, raster_ok)
        def build():
            for s_ in convs:
                m = s_["mod"]
                scale, shift = fold_bn(s_["bn"], m.bias if s_.get("bias") else None)
                w = m.weight.detach().reshape(-1, m.in_channels, m.out_channels).float().to(device)
                s_["w"], s_["scale"] = D.sparse_pack(s_["sp"], w, scale.to(device), s_["cin"])
                s_["shift"] = shift.to(device)
            return plan
        # one pack per structure list (see RPN._prepare).  The level grids do not depend on the pack and every call leaves
        # them clean: a new pack keeps them
        self._plan = self.packs.get(device, [m_ for s_ in convs for m_ in (s_["mod"], s_["bn"])],
                                    tuple((s_["sp"], s_["cin"], s_["cols"]) for s_ in convs), build)
        self.__dict__.setdefault("_levels", {})

    @staticmethod
    def _conv(step, b, feats, residual, out, io=0):
        """One fused sparse layer (conv + folded BN + optional residual + ReLU): plan step `step` on rulebook entry `b`."""
        D.sparse_launch(step["sp"], feats, b, step["w"], step["cin"], step["mod"].out_channels, step["scale"], step["shift"],
                        residual, True, out, io)

    def _level(self, shape, batch, device):
        key = tuple(int(s) for s in shape)
        lv = self._levels.get(key)
        if lv is None or lv.max_batch < batch:
            lv = _Level(key, max(batch, 1), device)
            self._levels[key] = lv
        return lv

    @staticmethod
    def _out_shape(shape, k, s, p):
        return [(shape[d] + 2 * p[d] - (k[d] - 1) - 1) // s[d] + 1 for d in range(3)]

    def build_rulebook(self, coords, batch_size, spatial_shape, frame_rows_max=0, neck_rows=False):
        """All index work of one batch.  It depends on the voxel coordinates only -- level grids,
        output sites of the strided convs (one small D2H each), every layer's tap-major table -- so
        the sweep can run it for batch i+1 on a side stream while batch i is being convolved.
        Returns ``dict(steps=[...])`` with one entry per item of the layer plan.  ``neck_rows``: the caller's neck can
        read the last level as ``detector_ops.BevRows``; where ``neck_rows_ok`` agrees the book carries the level's BEV
        row index (``bev_index``) instead of the zero-filled dense map (``dense``)."""
        if self.training:
            raise RuntimeError("al3d sparse encoder implements the eval() sweep only")
        dev = coords.device
        self._prepare(dev)
        st = _stream()
        coords = coords.to(torch.int32).contiguous()
        shape = [int(s) for s in spatial_shape]
        n = coords.shape[0]
        perm, raster_status = None, None
        if any(s_.get("sp") == "r16_f16x3" for s_ in self._plan):
            # the input level's rows renumbered in raster order (b, z, y, x): the order of a level's rows is free inside
            # the encoder (example["coordinates"] keeps the reference's first-appearance order), and raster order makes
            # the neighbour sets of consecutive rows contiguous index ranges (csrc/spconv_l0.hip)
            # (frame_rows_max > 0: the caller promises frame-sorted rows with at most that many rows per frame)
            perm, coords = D.raster_perm(coords, batch_size, shape, frame_rows_max)
            raster_status = D.raster_perm.last_status if frame_rows_max > 0 else None
        lv = self._level(shape, batch_size, dev)
        lib.call("al3d_sp_scatter_index", _ptr(coords), n, batch_size, lv.D, lv.H, lv.W, _ptr(lv.grid),
                 1, st)
        used = [(lv, coords, n)]
        tab, tab_key = None, None
        steps = []
        for pi, step in enumerate(self._plan):
            if step["kind"] == "stage_end":
                steps.append(dict(coords=coords, shape=shape, n=n))
                continue
            m = step["mod"]
            tiled = D.SPARSE[step["sp"]][2]
            if step["kind"] == "subm":
                # one table (and its side data) per level, shared by the level's layers
                key = (id(lv), m.kernel_size, tiled)
                if tab_key != key:
                    tab = D.sparse_table(tiled, coords, n, batch_size, (lv.D, lv.H, lv.W), lv.grid, m.kernel_size)
                    tab_key = key
            else:
                oshape = self._out_shape(shape, m.kernel_size, m.stride, m.padding)
                olv = self._level(oshape, batch_size, dev)
                # the order of the new level's rows: column by column when its layers run on the block-staged kernel
                # (csrc/spconv_blk.hip), raster otherwise
                nxt = next((s_ for s_ in self._plan[pi + 1:] if s_["kind"] != "stage_end"), None)
                cols = nxt is not None and nxt["kind"] == "subm" and nxt["cols"]
                ocoords = D.sparse_down_sites(coords, n, m.kernel_size, m.stride, m.padding, batch_size,
                                              (olv.D, olv.H, olv.W), olv.grid, cols)     # one small D2H per stage
                n_out = ocoords.shape[0]
                if raster_status is not None:    # the level-0 order's promise, checked where the stream is synchronised anyway
                    D.check_raster_status(raster_status)
                    raster_status = None
                if not cols and n_out > 0 and nxt is not None and nxt["kind"] == "subm" and \
                        int(np.prod(nxt["mod"].kernel_size)) == 27 and nxt["mod"].out_channels in D.MASK_SORT:
                    # rows of the new level grouped by tap mask inside windows of raster rows: more whole-tile tap skips
                    sorted_coords = torch.empty_like(ocoords)
                    msw = torch.empty(lib.load().al3d_sp_mask_window_sort_workspace_bytes(n_out), dtype=torch.uint8, device=dev)
                    lib.call("al3d_sp_mask_window_sort", _ptr(ocoords), n_out, batch_size, olv.D, olv.H, olv.W, _ptr(olv.grid),
                             D.MASK_SORT_WINDOWS.get(nxt["mod"].out_channels, D.MASK_SORT_WINDOW), _ptr(sorted_coords), _ptr(msw), st)
                    ocoords = sorted_coords
                used.append((olv, ocoords, n_out))
                tab = D.sparse_table(tiled, ocoords, n_out, batch_size, (lv.D, lv.H, lv.W), lv.grid, m.kernel_size,
                                     m.stride, m.padding)
                coords, n, shape, lv = ocoords, n_out, oshape, olv
                tab_key = None
            D.sparse_side(step["sp"], tab, step["cin"], m.out_channels)
            steps.append(tab)
        if raster_status is not None:
            D.check_raster_status(raster_status)
        for g, c, cnt in used:      # leave every level grid clean for the next call
            lib.call("al3d_sp_scatter_index", _ptr(c), cnt, batch_size, g.D, g.H, g.W, _ptr(g.grid), 0, st)
        # the zero-filled dense BEV buffer the last stage scatters into (537 MB at batch 32): also
        # coordinate-independent work that can be done ahead
        last_c = [st_["mod"].out_channels for st_ in self._plan if st_["kind"] != "stage_end"][-1]
        if neck_rows and D.neck_rows_ok("frag3x3", shape[0], last_c):
            # the index belongs to this batch's book, not to the resident level grids cleaned above: the neck reads it
            return dict(steps=steps, batch_size=batch_size, bev_index=D.bev_index(coords, n, batch_size, shape), perm=perm)
        dense = torch.zeros((batch_size, shape[1], shape[2], last_c * shape[0]), dtype=torch.float32, device=dev)
        return dict(steps=steps, batch_size=batch_size, dense=dense, perm=perm)

    def _run(self, feats, coords, batch_size, spatial_shape, book=None):
        """Returns (final SparseTensor, [SparseTensor per stage]).  ``book``: a rulebook built earlier
        by ``build_rulebook`` for these coordinates (else it is built here)."""
        if book is None:
            book = self.build_rulebook(coords, batch_size, spatial_shape)
        dev = feats.device
        feats = feats.float().contiguous()
        middle = []
        identity, identity_pair = None, False
        # f16x3: between two layers that both run a tiled matrix-core kernel the rows travel as pair rows (the
        # producer's epilogue splits once; csrc/sp_rows.h).  The first layer reads the VFE's f32 rows, the last one
        # writes f32 rows for the dense scatter.
        def pairable(step_):
            return D.SPROWS == "pair" and step_["kind"] != "stage_end" and D.SPARSE[step_["sp"]][2]
        convs = [s_ for s_ in self._plan if s_["kind"] != "stage_end"]
        ci, pair = 0, False
        perm = book.get("perm")
        for step, b in zip(self._plan, book["steps"]):
            if step["kind"] == "stage_end":
                middle.append(SparseTensor(feats, b["coords"], b["shape"], batch_size, pair_rows=pair))
                hook = getattr(self, "stage_hook", None)        # the sweep's pipeline: "stage k of the encoder is enqueued"
                if hook is not None:
                    hook(len(middle) - 1)
                continue
            m = step["mod"]
            r16 = step["sp"] == "r16_f16x3"
            if perm is not None or feats.shape[-1] != step["cin"]:
                assert not pair
                # the voxel features in the encoder's row order, zero-padded to the first layer's input width
                # (as pair rows when the first layer is an item-stream layer: AL3D_L0_ROWS)
                first_pair = D.L0_ROWS == "pair" and r16 and pairable(step)
                feats = D.rows_gather_pad(feats, perm, step["cin"], to_pair=first_pair)
                perm, pair = None, first_pair
            if step.get("block_start"):
                identity, identity_pair = feats, pair
            ok = pairable(step)
            assert ok or not pair, "pair rows reached a layer that cannot read them"
            # 16-channel rows stay f32: on the level-0 layers the pair-row epilogue costs more (+12 %) than the
            # consumers gain (-3 %); from 32 channels on the consumers are the LDS-DMA kernels (-5..10 %)
            # (the item-stream kernels of level 0 are bound by instruction issue, the split is a third of their vector
            # instructions: there 16-channel rows travel as pair rows too)
            out_pair = ok and ci + 1 < len(convs) and pairable(convs[ci + 1]) and (
                m.out_channels >= 32 or (D.L0_ROWS == "pair" and r16 and convs[ci + 1]["sp"] == "r16_f16x3"))
            res = identity if step.get("residual") else None
            io = ((D.IO_IN_PAIR if pair else 0) | (D.IO_OUT_PAIR if out_pair else 0) |
                  (D.IO_RES_PAIR if (res is not None and identity_pair) else 0))
            out = torch.empty((b["n"], m.out_channels), dtype=torch.float32, device=dev)
            self._conv(step, b, feats, res, out, io)
            feats, pair = out, out_pair
            ci += 1
        assert not pair
        last = middle[-1]
        return SparseTensor(feats, last.indices, last.spatial_shape, batch_size), middle

    def rulebook_for(self, coors, batch_size, input_shape, frame_rows_max=0, neck_rows=False):
        return self.build_rulebook(coors, batch_size, np.array(input_shape[::-1]) + [1, 0, 0], frame_rows_max, neck_rows)

    def _forward(self, voxel_features, coors, batch_size, input_shape, book=None, frame_rows_max=0, neck_rows=False):
        """-> (dense NHWC map or ``detector_ops.BevRows``, the stages' SparseTensors) on the reference's sparse shape
        ``input_shape[::-1] + [1, 0, 0]``."""
        sparse_shape = np.array(input_shape[::-1]) + [1, 0, 0]
        if book is None:
            book = self.build_rulebook(coors, batch_size, sparse_shape, frame_rows_max, neck_rows)
        final, middle = self._run(voxel_features, coors, batch_size, sparse_shape, book=book)
        index = book.get("bev_index")
        if index is not None:
            rows = D.BevRows(final.features, final.indices, index)
            return (rows if neck_rows else rows.dense()), middle
        return self.dense_nhwc(final, out=book.pop("dense", None)), middle

    @staticmethod
    def dense_nhwc(sp, out=None):
        """``ret.dense()`` + ``view(N, C*D, H, W)`` in NHWC: [B, H, W, C*D], channel = c*D + z.
        ``out``: an already zero-filled buffer of that shape (the rulebook pass prepares one)."""
        D, H, W = sp.spatial_shape
        C = sp.features.shape[1]
        if out is None or tuple(out.shape) != (sp.batch_size, H, W, C * D):
            out = torch.zeros((sp.batch_size, H, W, C * D), dtype=torch.float32, device=sp.features.device)
        lib.call("al3d_sp_to_dense_nhwc", _ptr(sp.features), _ptr(sp.indices), sp.features.shape[0], C,
                 sp.batch_size, D, H, W, _ptr(out), _stream())
        return out


@BACKBONES.register_module
class FPNSpMiddleResNetFHD(_SparseEncoderBase):
    def __init__(self, num_input_features=128, norm_cfg=None, name="SpMiddleResNetFHD", **kwargs):
        super().__init__()
        self.name = name
        self.middle_conv0 = nn.Sequential(
            SubMConv3d(num_input_features, 16, 3, bias=False, indice_key="res0"), _bn(16), nn.ReLU(),
            SparseBasicBlock(16, 16, indice_key="res0"), SparseBasicBlock(16, 16, indice_key="res0"),
            SparseConv3d(16, 32, 3, 2, padding=1, bias=False), _bn(32), nn.ReLU())
        self.middle_conv1 = nn.Sequential(
            SparseBasicBlock(32, 32, indice_key="res1"), SparseBasicBlock(32, 32, indice_key="res1"),
            SparseConv3d(32, 64, 3, 2, padding=1, bias=False), _bn(64), nn.ReLU())
        self.middle_conv2 = nn.Sequential(
            SparseBasicBlock(64, 64, indice_key="res2"), SparseBasicBlock(64, 64, indice_key="res2"),
            SparseConv3d(64, 128, 3, 2, padding=[0, 1, 1], bias=False), _bn(128), nn.ReLU())
        self.middle_conv3 = nn.Sequential(
            SparseBasicBlock(128, 128, indice_key="res3"), SparseBasicBlock(128, 128, indice_key="res3"),
            SparseConv3d(128, 128, (3, 1, 1), (2, 1, 1), bias=False), _bn(128), nn.ReLU())

    def _stages(self):
        return [self.middle_conv0, self.middle_conv1, self.middle_conv2, self.middle_conv3]

    def forward(self, voxel_features, coors, batch_size, input_shape, book=None, frame_rows_max=0, neck_rows=False):
        """-> (dense NHWC [B,128,128,256], middle list of 4 SparseTensor) -- the reference
        returns NCHW (scn.py:371-392); this build keeps activations channels-last.  ``neck_rows=True`` (a caller whose
        neck takes it): a ``detector_ops.BevRows`` in place of the dense map when the book carries the row index."""
        return self._forward(voxel_features, coors, batch_size, input_shape, book, frame_rows_max, neck_rows)


class _SingleStageEncoder(_SparseEncoderBase):
    """det3d's encoders that are ONE ``middle_conv`` sequence (scn.py:100-205, 395-457): the state-dict keys are the
    reference's ``middle_conv.<i>.*``.  Same call as the FPN encoder (``book``, ``frame_rows_max``, ``neck_rows``,
    ``rulebook_for``), but like the reference they return the dense map alone -- there is no ``middle``."""

    def _stages(self):
        return [self.middle_conv]

    def forward(self, voxel_features, coors, batch_size, input_shape, book=None, frame_rows_max=0, neck_rows=False):
        """-> dense NHWC [B, H, W, C*D] with channel = c*D + z (the reference returns NCHW, scn.py:192-205), or a
        ``detector_ops.BevRows`` under ``neck_rows=True`` when the book carries the row index."""
        return self._forward(voxel_features, coors, batch_size, input_shape, book, frame_rows_max, neck_rows)[0]


@BACKBONES.register_module
class SpMiddleResNetFHD(_SingleStageEncoder):
    """The residual encoder without the FPN taps (reference scn.py:395-457; the model of ``cbgs_full.py``): the layers
    of ``FPNSpMiddleResNetFHD`` in one sequence -- convs at ``middle_conv.{0,5,10,15,20}``, ``SparseBasicBlock`` s at
    ``{3,4,8,9,13,14,18,19}``."""

    def __init__(self, num_input_features=128, norm_cfg=None, name="SpMiddleResNetFHD", **kwargs):
        super().__init__()
        self.name = name
        self.middle_conv = nn.Sequential(
            SubMConv3d(num_input_features, 16, 3, bias=False, indice_key="res0"), _bn(16), nn.ReLU(),
            SparseBasicBlock(16, 16, indice_key="res0"), SparseBasicBlock(16, 16, indice_key="res0"),
            SparseConv3d(16, 32, 3, 2, padding=1, bias=False), _bn(32), nn.ReLU(),
            SparseBasicBlock(32, 32, indice_key="res1"), SparseBasicBlock(32, 32, indice_key="res1"),
            SparseConv3d(32, 64, 3, 2, padding=1, bias=False), _bn(64), nn.ReLU(),
            SparseBasicBlock(64, 64, indice_key="res2"), SparseBasicBlock(64, 64, indice_key="res2"),
            SparseConv3d(64, 128, 3, 2, padding=[0, 1, 1], bias=False), _bn(128), nn.ReLU(),
            SparseBasicBlock(128, 128, indice_key="res3"), SparseBasicBlock(128, 128, indice_key="res3"),
            SparseConv3d(128, 128, (3, 1, 1), (2, 1, 1), bias=False), _bn(128), nn.ReLU())


@BACKBONES.register_module
class SpMiddleFHD(_SingleStageEncoder):
    """SECOND's plain encoder (reference scn.py:100-205): fourteen bias-free conv + BN + ReLU triples at
    ``middle_conv.{0,3,...,39}``, channels 16,16 | 32,32,32 | 64,64,64,64 | 64,64,64,64; the dense map has
    64 * 2 = 128 channels."""

    def __init__(self, num_input_features=128, norm_cfg=None, name="SpMiddleFHD", **kwargs):
        super().__init__()
        self.name = name

        def subm(cin, cout, key):
            return [SubMConv3d(cin, cout, 3, bias=False, indice_key=key), _bn(cout), nn.ReLU()]

        def down(cin, cout, k=3, s=2, p=1):
            return [SparseConv3d(cin, cout, k, s, padding=p, bias=False), _bn(cout), nn.ReLU()]

        self.middle_conv = nn.Sequential(
            *subm(num_input_features, 16, "subm0"), *subm(16, 16, "subm0"),
            *down(16, 32), *subm(32, 32, "subm1"), *subm(32, 32, "subm1"),
            *down(32, 64), *subm(64, 64, "subm2"), *subm(64, 64, "subm2"), *subm(64, 64, "subm2"),
            *down(64, 64, p=[0, 1, 1]), *subm(64, 64, "subm3"), *subm(64, 64, "subm3"), *subm(64, 64, "subm3"),
            *down(64, 64, (3, 1, 1), (2, 1, 1), 0))


@BACKBONES.register_module
class PointPillarsScatter(nn.Module):
    """Pillar rows -> BEV pseudo image (det3d/models/readers/pillar_encoder.py:155-211; BEVFusion's
    bevfusion/mmdet3d/models/backbones/pillar_encoder.py:185-240 under ``in_channels`` / ``output_shape``).

    ``forward(voxel_features [M,C], coords [M,4] (b,z,y,x), batch_size, input_shape)`` -> this build's channels-last
    canvas ``[B, ny, nx, C]`` (H = y, W = x), zero where there is no pillar; ``input_shape`` is the voxel grid
    (nx, ny, nz), or ``output_shape`` (nx, ny) when None.  One ``al3d_pillar_scatter_nhwc_f32`` launch.  The
    ``PointPillars`` detector does not call it: its reader writes the canvas directly."""

    def __init__(self, num_input_features=64, norm_cfg=None, name="PointPillarsScatter", in_channels=None,
                 output_shape=None, **kwargs):
        super().__init__()
        self.name = name
        self.nchannels = num_input_features if in_channels is None else in_channels
        self.output_shape = output_shape

    def forward(self, voxel_features, coords, batch_size, input_shape=None):
        shape = input_shape if input_shape is not None else self.output_shape
        if shape is None:
            raise lib.Al3dError("PointPillarsScatter: no input_shape and no output_shape")
        if voxel_features.shape[-1] != self.nchannels:
            raise lib.Al3dError(f"PointPillarsScatter: {voxel_features.shape[-1]} channels, built for {self.nchannels}")
        nx, ny = int(shape[0]), int(shape[1])
        return D.pillar_scatter(voxel_features, coords, int(batch_size), ny, nx)
