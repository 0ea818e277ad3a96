"""CPU suite: when the encoder -> neck hand-over may travel as rows (``detector_ops.BevRows``) and when the dense path is
taken.  The rows form needs f16x3, a first neck conv on the streamed 3x3 kernel ("frag3x3"), two z levels, row channels
that are a multiple of 8 and ``AL3D_NECK_IN=rows``; everywhere else the neck runs on the dense tensor, taken from the
object's ``dense()`` when it was handed one."""
import pytest
import torch


def _set(monkeypatch, math="f16x3", dense="auto", neck_in="rows"):
    from al3d import detector_ops as D
    monkeypatch.setattr(D, "MATH", math)
    monkeypatch.setattr(D, "DENSE", dense)
    monkeypatch.setattr(D, "NECK_IN", neck_in)
    monkeypatch.setattr(D, "GAP", "standalone")          # no fused-GAP launches in the stubbed forward
    return D


def test_knob_values():
    from al3d import detector_ops as D
    assert D.NECK_IN in ("rows", "dense")


@pytest.mark.parametrize("math,neck_in,kind,depth,channels,ok", [
    ("f16x3", "rows", "frag3x3", 2, 128, True),
    ("f16x3", "rows", "frag3x3", 2, 8, True),
    ("bf16x6", "rows", "frag3x3", 2, 128, False),
    ("bf16x6", "rows", "bf16x6", 2, 128, False),
    ("f32", "rows", "f32", 2, 128, False),
    ("f16x3", "dense", "frag3x3", 2, 128, False),
    ("f16x3", "rows", "dma", 2, 128, False),
    ("f16x3", "rows", "f16x3", 2, 128, False),
    ("f16x3", "rows", "frag16", 2, 128, False),
    ("f16x3", "rows", "wino", 2, 128, False),
    ("f16x3", "rows", "frag3x3", 1, 128, False),
    ("f16x3", "rows", "frag3x3", 3, 128, False),
    ("f16x3", "rows", "frag3x3", 2, 12, False),
])
def test_eligibility_rule(monkeypatch, math, neck_in, kind, depth, channels, ok):
    D = _set(monkeypatch, math=math, neck_in=neck_in)
    assert D.neck_rows_ok(kind, depth, channels) is ok


def _rpn(first_stride=1, cin=256):
    from al3d.models.necks import RPN
    return RPN(layer_nums=[1], ds_layer_strides=[first_stride], ds_num_filters=[128], us_layer_strides=[1],
               us_num_filters=[128], num_input_features=cin).eval()


@pytest.mark.parametrize("math,dense,neck_in,stride,cin,ok", [
    ("f16x3", "auto", "rows", 1, 256, True),
    ("f16x3", "auto", "dense", 1, 256, False),
    ("bf16x6", "auto", "rows", 1, 256, False),
    ("f32", "auto", "rows", 1, 256, False),
    ("f16x3", "lds", "rows", 1, 256, False),         # LDS-staged kernels: the first conv is not the streamed one
    ("f16x3", "wino", "rows", 1, 256, False),
    ("f16x3", "frag16", "rows", 1, 256, False),
    ("f16x3", "auto", "rows", 2, 256, False),        # strided entry conv: the LDS-DMA kernel
    ("f16x3", "auto", "rows", 1, 80, False),         # Cin no multiple of 32: not a frag3x3 layer
])
def test_neck_says_whether_it_takes_rows(monkeypatch, math, dense, neck_in, stride, cin, ok):
    _set(monkeypatch, math=math, dense=dense, neck_in=neck_in)
    assert _rpn(stride, cin).rows_input_ok() is ok


class _FakeRows:
    """A BevRows on the CPU whose dense() is counted."""

    def __new__(cls, depth=2, channels=128):
        from al3d import detector_ops as D

        class Counted(D.BevRows):
            calls = 0

            def dense(self):
                type(self).calls += 1
                return torch.zeros(self.shape)
        index = torch.full((1, 8, 8, depth), -1, dtype=torch.int32)
        return Counted(torch.zeros((0, channels)), torch.zeros((0, 4), dtype=torch.int32), index)


def _stub_forward(monkeypatch, D, neck, first_kind):
    """RPN.forward without a device: the packs are placeholders of the given kinds, conv2d_nhwc records its input."""
    cin = neck._num_input_features
    vec = torch.ones(128)
    neck._blocks_p = [[dict(w=D.F16x3Packed(first_kind, None, 128, 9, cin), scale=vec, shift=vec, k=3, s=1, p=1),
                       dict(w=D.F16x3Packed("frag3x3", None, 128, 9, 128), scale=vec, shift=vec, k=3, s=1, p=1)]]
    neck._deblocks_p = [dict(deconv=False, w=D.F16x3Packed("dma", None, 128, 1, 128), scale=vec, shift=vec, k=1, s=1)]
    monkeypatch.setattr(type(neck), "_prepare", lambda self, device: None)
    inputs = []

    def conv(x, w, scale, shift, k, s, p, relu, out=None, coff=0, gap=None, io=0):
        inputs.append(x)
        return out if out is not None else torch.zeros(tuple(x.shape[:3]) + (w.cout,))
    monkeypatch.setattr(D, "conv2d_nhwc", conv)
    return inputs


@pytest.mark.parametrize("math,first_kind,depth,channels,takes_rows", [
    ("f16x3", "frag3x3", 2, 128, True),
    ("bf16x6", "frag3x3", 2, 128, False),            # the AL3D_MATH=auto re-run flips MATH under a live detector
    ("f16x3", "dma", 2, 128, False),
    ("f16x3", "f16x3", 2, 128, False),
    ("f16x3", "frag3x3", 3, 128, False),
    ("f16x3", "frag3x3", 1, 128, False),
])
def test_neck_forward_routes_rows_or_dense(monkeypatch, math, first_kind, depth, channels, takes_rows):
    D = _set(monkeypatch, math=math)
    neck = _rpn(1, channels * depth)
    inputs = _stub_forward(monkeypatch, D, neck, first_kind)
    x = _FakeRows(depth, channels)
    out = neck(x)
    assert tuple(out.shape) == (1, 8, 8, 128)
    assert len(inputs) == 3                             # entry conv, one 3x3, the 1x1 deblock: all through D.conv2d_nhwc
    if takes_rows:
        assert inputs[0] is x and type(x).calls == 0
    else:
        assert isinstance(inputs[0], torch.Tensor) and type(x).calls == 1
        assert tuple(inputs[0].shape) == tuple(x.shape)
    assert all(isinstance(t, torch.Tensor) for t in inputs[1:])


def test_dense_launch_refuses_rows_it_cannot_read(monkeypatch):
    from al3d import lib
    D = _set(monkeypatch, math="bf16x6")
    x = _FakeRows()
    with pytest.raises(lib.Al3dError):
        D.conv2d_nhwc(x, D.F16x3Packed("frag3x3", None, 128, 9, 256), torch.ones(128), None, 3, 1, 1, True)


def test_detector_asks_for_rows_only_for_its_own_neck(monkeypatch):
    from al3d.models.backbones import FPNSpMiddleResNetFHD
    from al3d.models.detectors import FPNVoxelNet
    D = _set(monkeypatch)

    class Det(FPNVoxelNet):
        def __init__(self, neck):
            torch.nn.Module.__init__(self)
            self.backbone, self.neck = FPNSpMiddleResNetFHD(num_input_features=5), neck
    det = Det(_rpn())
    assert det._neck_rows() is True
    monkeypatch.setattr(D, "MATH", "bf16x6")
    assert det._neck_rows() is False
    monkeypatch.setattr(D, "MATH", "f16x3")
    det.neck_rows = False                               # what BEVFusion sets on its lidar half: the fuser reads the dense map
    assert det._neck_rows() is False
    assert Det(_rpn(first_stride=2))._neck_rows() is False
    assert Det(torch.nn.Identity())._neck_rows() is False
