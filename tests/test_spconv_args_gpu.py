"""GPU suite: the host argument contract of the f16x3 sparse-conv entry points (csrc/spconv_{wave,glds,rng,blk,l0}.hip).

Every rejection below happens in the entry point's checks, before anything is launched: a wrong pitch, a missing scale,
io flags out of range, a missing tile mask / side table, a channel pair without a kernel, K = 26 where the structure is
built for 27 taps.  n_out = 0 returns OK before the pointers are looked at.  The message of a rejection starts with the
name the library reports for the entry point: its own, or -- for the checks the plain and the _io / _tiles_io entry
points share -- the name of the plain one."""
import numpy as np
import pytest
import torch

from test_detector_oracle import random_sparse

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N_ROWS = 33                      # two 32-row tiles, the second ragged

# structure -> (entry point, the name its shared checks report, K must be 27)
ENTRIES = {
    "wave2_f16x3_tiles": ("al3d_sp_conv_wave2_f16x3_tiles_io", "al3d_sp_conv_wave2_f16x3", False),
    "glds_f16x3": ("al3d_sp_conv_glds_f16x3_io", "al3d_sp_conv_glds_f16x3", False),
    "rng_f16x3": ("al3d_sp_conv_rng_f16x3", "al3d_sp_conv_rng_f16x3", True),
    "blk_f16x3": ("al3d_sp_conv_blk_f16x3", "al3d_sp_conv_blk_f16x3", True),
    "r16_f16x3": ("al3d_sp_conv_r16_f16x3", "al3d_sp_conv_r16_f16x3", True),
}
STRUCTURES = list(ENTRIES)


class _Layer:
    """One tiny valid submanifold layer of a structure and the argument list of its entry point, by name."""

    def __init__(self, name, c):
        from al3d import detector_ops as D
        from al3d.selector_ops import _ptr, _stream
        self.name, self.fn, self.c = name, ENTRIES[name][0], c
        rng = np.random.default_rng(5)
        batch, dims = 1, [3, 5, 4]
        feats, coords = random_sparse(rng, batch, dims, N_ROWS, c)
        order = np.lexsort((coords[:, 3], coords[:, 2], coords[:, 1], coords[:, 0]))      # raster order (b, z, y, x)
        self.feats = torch.from_numpy(feats[order]).to(DEV)
        self.coords = torch.from_numpy(np.ascontiguousarray(coords[order])).to(DEV)
        w = torch.from_numpy((rng.normal(size=(27, c, c)) / np.sqrt(c * 9)).astype(np.float32)).to(DEV)
        scale = torch.from_numpy(rng.uniform(0.5, 1.5, c).astype(np.float32)).to(DEV)
        self.shift = torch.from_numpy(rng.normal(0, 0.1, c).astype(np.float32)).to(DEV)
        self.w, self.scale = D.sparse_pack(name, w, scale)
        grid = torch.full((batch * dims[0] * dims[1] * dims[2],), -1, dtype=torch.int32, device=DEV)
        D.lib.call("al3d_sp_scatter_index", _ptr(self.coords), N_ROWS, batch, *dims, _ptr(grid), 1, _stream())
        self.tab = D.sparse_table(True, self.coords, N_ROWS, batch, dims, grid, [3, 3, 3])
        D.sparse_side(name, self.tab, c, c)
        self.out = torch.zeros((N_ROWS, c), dtype=torch.float32, device=DEV)
        side = D.SPARSE[name][3]
        self.side_keys = {None: ["tmask"], "trng": ["tmask", "trng"], "plan": ["tmask", "hdr", "rows", "loc"],
                          "items": ["items", "first"]}[side]
        side_ptrs = [_ptr(t) for t in D._SIDE_ARGS[side](self.tab)]
        # the argument list in the order of include/al3d.h (sparse_launch's)
        self.args = dict(fin=_ptr(self.feats), nbr=_ptr(self.tab["nbr"]), pitch=self.tab["nbr"].shape[1],
                         **dict(zip(self.side_keys, side_ptrs)), K=27, wgt=_ptr(self.w), cin=c, cout=c,
                         scale=_ptr(self.scale), shift=_ptr(self.shift), residual=None, relu=1, fout=_ptr(self.out),
                         n_out=N_ROWS, io=0)
        if side == "items":
            self.args["tiles_per_wave"] = 0
        self.args["stream"] = _stream()

    def call(self, **changed):
        from al3d import lib
        lib.call(self.fn, *{**self.args, **changed}.values())


@pytest.fixture(scope="module")
def layers():
    made = {name: _Layer(name, 16 if name == "r16_f16x3" else 32) for name in STRUCTURES}
    made["reference 16"] = _Layer("wave2_f16x3_tiles", 16)          # the 16 -> 16 layer through the register-gather kernel
    made["reference 32"] = made["wave2_f16x3_tiles"]
    return made


def _rejected(layer, fragment, **changed):
    """The call raises Al3dError; the library's message names the entry point and holds `fragment`."""
    from al3d import lib
    with pytest.raises(lib.Al3dError) as err:
        layer.call(**changed)
    msg = str(err.value).split(": ", 1)[1]                # lib.check: "<entry> failed with status <n>: <library message>"
    entry, shared, _ = ENTRIES[layer.name]
    assert msg.startswith(entry + ":") or msg.startswith(shared + ":"), msg
    assert fragment in msg, msg


@pytest.mark.parametrize("name", STRUCTURES)
def test_valid_tiny_layer(layers, name):
    """33 rows (a ragged second tile) run, and give the register-gather kernel's bits."""
    L, ref = layers[name], layers[f"reference {layers[name].c}"]
    for layer in (L, ref):
        layer.out.fill_(float("nan"))
        layer.call()
    torch.cuda.synchronize()
    got = L.out.cpu().numpy()
    assert np.isfinite(got).all() and np.abs(got).max() > 0
    assert np.array_equal(ref.out.cpu().numpy().view(np.int32), got.view(np.int32))


@pytest.mark.parametrize("name", STRUCTURES)
def test_pitch_not_a_multiple_of_256(layers, name):
    frag = "needs a tiled rulebook" if name == "wave2_f16x3_tiles" else "nbr_pitch must be al3d_sp_table_pitch(n_out)"
    _rejected(layers[name], frag, pitch=layers[name].args["pitch"] + 32)


@pytest.mark.parametrize("name", STRUCTURES)
def test_missing_scale(layers, name):
    _rejected(layers[name], "scale carries the weight exponent and is required", scale=None)


@pytest.mark.parametrize("name", STRUCTURES)
def test_io_out_of_range(layers, name):
    _rejected(layers[name], "bad io flags", io=8)


@pytest.mark.parametrize("name", STRUCTURES)
def test_missing_tile_mask_or_side_table(layers, name):
    L = layers[name]
    for key in L.side_keys:
        frag = "needs a tiled rulebook" if name == "wave2_f16x3_tiles" else "null pointer"
        _rejected(L, frag, **{key: None})


@pytest.mark.parametrize("name", STRUCTURES)
def test_unsupported_channel_pair(layers, name):
    L = layers[name]
    if name == "r16_f16x3":
        _rejected(L, "no kernel for Cout=48", cout=48)
        _rejected(L, "16 input channels only", cin=32)
    else:
        frag = "unsupported channel pair 32 -> 48" if name in ("wave2_f16x3_tiles", "glds_f16x3") else "no kernel for Cin=32 Cout=48"
        _rejected(L, frag, cout=48)


@pytest.mark.parametrize("name", [n for n in STRUCTURES if ENTRIES[n][2]])
def test_k_26_where_27_is_required(layers, name):
    _rejected(layers[name], "27-tap", K=26)


@pytest.mark.parametrize("name", STRUCTURES)
def test_no_rows_returns_ok_before_the_pointers(layers, name):
    """n_out = 0: OK with every pointer null.  (The register-gather entry point checks that it was handed a tiled
    rulebook -- mask and pitch -- before anything else: it keeps its mask.)"""
    L = layers[name]
    nulls = {k: None for k in ["fin", "nbr", "wgt", "scale", "shift", "fout"] + L.side_keys}
    if name == "wave2_f16x3_tiles":
        del nulls["tmask"]
    L.call(n_out=0, pitch=0, **nulls)
