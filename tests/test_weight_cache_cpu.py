"""The one packed-weight cache (``al3d.weight_cache``) and the one conv + BN fold (``detector_ops.fold_conv_bn``): pure
torch, no library call."""
import pytest
import torch
import torch.nn.functional as F
from torch import nn


class _Counter:
    def __init__(self):
        self.n = 0

    def __call__(self):
        self.n += 1
        return object()


def _pair(seed=0):
    torch.manual_seed(seed)
    return nn.Conv2d(3, 4, 3, padding=1), nn.BatchNorm2d(4).eval()


def test_versions_reads_modules_and_tensors_and_skips_none():
    from al3d.weight_cache import versions
    conv, bn = _pair()
    t = torch.zeros(3)
    v = versions(conv, None, bn, t)
    own = [conv.weight, conv.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.num_batches_tracked, t]
    assert v == tuple((p.data_ptr(), p._version) for p in own)
    assert versions(nn.Sequential(conv)) == ()                      # recurse=False: a container has no tensors of its own
    assert versions(conv, None) == versions(conv)


def test_same_stamp_and_variant_builds_once():
    from al3d.weight_cache import PackCache
    conv, bn = _pair()
    cache, build = PackCache(), _Counter()
    a = cache.get("cpu", (conv, bn), "A", build)
    assert cache.get(torch.device("cpu"), (conv, bn), "A", build) is a and build.n == 1
    assert cache.get("cpu", (conv, bn), build=build) is cache.get("cpu", (conv, bn), None, build) and build.n == 2


def test_one_pack_per_variant():
    from al3d.weight_cache import PackCache
    conv, bn = _pair()
    cache, build = PackCache(), _Counter()
    a = cache.get("cpu", (conv, bn), "A", build)
    b = cache.get("cpu", (conv, bn), ("B", 1), build)
    assert cache.get("cpu", (conv, bn), "A", build) is a and a is not b and build.n == 2


def _edit_weight(conv, bn):
    with torch.no_grad():
        conv.weight.add_(1)


def _load(conv, bn):
    conv.load_state_dict(_pair(1)[0].state_dict())


def _edit_mean(conv, bn):
    bn.running_mean.add_(0.5)


def _new_storage(conv, bn):
    conv.double().float()


@pytest.mark.parametrize("write", [_edit_weight, _load, _edit_mean, _new_storage])
def test_a_written_parameter_or_buffer_drops_every_variant(write):
    from al3d.weight_cache import PackCache
    conv, bn = _pair()
    cache, build = PackCache(), _Counter()
    a, b = cache.get("cpu", (conv, bn), "A", build), cache.get("cpu", (conv, bn), "B", build)
    write(conv, bn)
    a2 = cache.get("cpu", (conv, bn), "A", build)
    assert a2 is not a and build.n == 3
    assert cache.get("cpu", (conv, bn), "B", build) is not b and build.n == 4          # the other variant went too
    assert cache.get("cpu", (conv, bn), "A", build) is a2 and build.n == 4


def test_another_device_and_clear_rebuild():
    from al3d.weight_cache import PackCache
    conv, bn = _pair()
    cache, build = PackCache(), _Counter()
    a = cache.get("cpu", (conv, bn), "A", build)
    m = cache.get("meta", (conv, bn), "A", build)                    # the stamp holds the device, nothing is moved
    assert m is not a and build.n == 2
    assert cache.get("cpu", (conv, bn), "A", build) is not a and build.n == 3
    cache.clear()
    cache.get("cpu", (conv, bn), "A", build)
    assert build.n == 4


def test_none_among_the_sources_is_ignored():
    from al3d.weight_cache import PackCache
    conv, _ = _pair()
    cache, build = PackCache(), _Counter()
    a = cache.get("cpu", (conv, None), "A", build)
    assert cache.get("cpu", (conv,), "A", build) is a and build.n == 1


# ------------------------------------------------------------------ fold_conv_bn against torch in float64
def _seeded(mods, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in mods:
            for t in list(m.parameters()) + [b for b in m.buffers() if b.dtype.is_floating_point]:
                t.copy_(torch.rand(t.shape, generator=g) + 0.5 if t.dim() == 1 else torch.randn(t.shape, generator=g) * 0.3)
    return mods


def _unpacked(w, k):
    """[Cout, taps, Cin] -> [Cout, Cin, k, k]."""
    return w.reshape(w.shape[0], k, k, w.shape[2]).permute(0, 3, 1, 2).double()


def _check(got, want):
    err = float((got - want).abs().max())
    assert err <= 1e-5 * float(want.abs().max()), err


def _x(cin, seed=5):
    return torch.randn(2, cin, 5, 6, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


@pytest.mark.parametrize("cin", [3, 16])
@pytest.mark.parametrize("with_bn", [True, False])
def test_fold_conv_with_bias_and_optional_bn(cin, with_bn):
    from al3d import detector_ops as D
    conv, bn = _seeded([nn.Conv2d(cin, 8, 3, padding=1), nn.BatchNorm2d(8).eval()], cin)
    w, scale, shift = D.fold_conv_bn([(conv, bn if with_bn else None)])
    assert w.shape == (8, 9, cin) and w.dtype == scale.dtype == shift.dtype == torch.float32
    if not with_bn:
        assert torch.equal(scale, torch.ones(8)) and torch.equal(shift, conv.bias.detach())
    x = _x(cin)
    want = conv.double()(x)
    want = bn.double()(want) if with_bn else want
    got = F.conv2d(x, _unpacked(w, 3), padding=1) * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1)
    _check(got, want.detach())


@pytest.mark.parametrize("cin", [3, 16])
def test_fold_two_convs_side_by_side(cin):
    from al3d import detector_ops as D
    c0, b0, c1 = _seeded([nn.Conv2d(cin, 8, 3, padding=1, bias=False), nn.BatchNorm2d(8).eval(), nn.Conv2d(cin, 5, 3, padding=1)], 7)
    w, scale, shift = D.fold_conv_bn([(c0, b0), (c1, None)])
    assert w.shape == (13, 9, cin)
    x = _x(cin)
    want = torch.cat([b0.double()(c0.double()(x)), c1.double()(x)], dim=1).detach()
    got = F.conv2d(x, _unpacked(w, 3), padding=1) * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1)
    _check(got, want)


@pytest.mark.parametrize("cin", [3, 16])
def test_fold_with_the_spatial_axes_swapped(cin):
    """The map is stored [y, x], the weights are [x, y]: the folded kernel on the transposed map gives the transposed result."""
    from al3d import detector_ops as D
    conv, bn = _seeded([nn.Conv2d(cin, 8, 3, padding=1), nn.BatchNorm2d(8).eval()], 8)
    w, scale, shift = D.fold_conv_bn([(conv, bn)], swap_hw=True)
    x = _x(cin)
    want = bn.double()(conv.double()(x)).detach().transpose(2, 3)
    got = F.conv2d(x.transpose(2, 3), _unpacked(w, 3), padding=1) * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1)
    _check(got, want)


@pytest.mark.parametrize("cin,first", [(3, 1), (16, 6)])
def test_fold_with_rotated_input_channels(cin, first):
    from al3d import detector_ops as D
    conv, bn = _seeded([nn.Conv2d(cin, 8, 1, bias=False), nn.BatchNorm2d(8).eval()], 9)
    w, scale, shift = D.fold_conv_bn([(conv, bn)], first=first)
    x = _x(cin)
    want = bn.double()(conv.double()(x)).detach()
    rotated = torch.cat([x[:, first:], x[:, :first]], dim=1)         # the map the layer is handed
    got = F.conv2d(rotated, _unpacked(w, 1)) * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1)
    _check(got, want)


def test_fold_pads_cin_to_a_multiple_of_16():
    from al3d import detector_ops as D
    conv, bn = _seeded([nn.Conv2d(3, 8, 3, padding=1), nn.BatchNorm2d(8).eval()], 10)
    plain = D.fold_conv_bn([(conv, bn)])
    w, scale, shift = D.fold_conv_bn([(conv, bn)], pad_cin=True)
    assert w.shape == (8, 9, 16) and torch.equal(w[..., :3], plain[0]) and not w[..., 3:].any()
    assert torch.equal(scale, plain[1]) and torch.equal(shift, plain[2])
    c16 = nn.Conv2d(16, 8, 3, padding=1)
    assert D.fold_conv_bn([(c16, None)], pad_cin=True)[0].shape == (8, 9, 16)
    x = _x(3)
    want = bn.double()(conv.double()(x)).detach()
    got = F.conv2d(F.pad(x, (0, 0, 0, 0, 0, 13)), _unpacked(w, 3), padding=1) * scale.double().view(1, -1, 1, 1) + \
        shift.double().view(1, -1, 1, 1)
    _check(got, want)


@pytest.mark.parametrize("cin", [3, 16])
def test_fold_the_2x2_deconvolution(cin):
    from al3d import detector_ops as D
    up, bn = _seeded([nn.ConvTranspose2d(cin, 8, 2, stride=2, bias=False), nn.BatchNorm2d(8).eval()], 11)
    w, scale, shift = D.fold_conv_bn([(up, bn)], deconv=True)
    assert w.shape == (8, 4, cin)                                    # [Cout, tap = dy * 2 + dx, Cin]
    x = _x(cin)
    want = bn.double()(up.double()(x)).detach()
    back = w.double().reshape(8, 2, 2, cin).permute(3, 0, 1, 2)      # -> ConvTranspose2d's [Cin, Cout, 2, 2]
    got = F.conv_transpose2d(x, back, stride=2) * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1)
    _check(got, want)
