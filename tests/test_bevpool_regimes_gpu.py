"""GPU suite: csrc/bev_pool.hip's pooling kernels at every data-dependent branch, bit for bit against the CPU oracle
(both add a cell's points in ascending point index; the oracle itself is pinned to a torch index_add_ statement on these
very inputs by tests/test_bevpool_oracle.py).

Inputs come from tests/bevpool_cases.py: exact member counts on consecutive cell ids, so that one 76 k-point input
holds the three ways a member list is ordered (rank counting in the wave for len <= 128, bitonic sort in LDS for
128 < len <= 8192, rank counting by a workgroup beyond), both boundaries (128 | 129, 8192 | 8193), an empty cell, and --
at 1, 2, 3 and 4 cells per wave of bev_sum_vec_kernel (C = 256, 128, 80, <= 64) -- waves whose cells are of different
regimes.  Every comparison is of the int32 view: a dropped, duplicated or reordered point changes low bits of a sum of
normal variates.

What a wrong kernel would trip (read against the code, not tried):
  * rank counting for len <= 128 (bev_sum_kernel's loop, bev_sum_vec_kernel's LDS loop): cells 1, 3, 5, 7, 11, 12 of sample 0
    and every background cell differ from the oracle in test_materialised_pool_every_regime (generic: C = 6, 260; float4:
    C = 80, 4, 128, 256) and in test_fused_lss_pool_every_regime;
  * the bitonic sort of bev_sort_long_kernel (padding, direction bit, the store of the first `len` keys): cells 4 (129),
    6 (8192), 10 (300) of sample 0 and cells 37, 38, 500, 959 of sample 1 differ in the same assertions;
  * the rank-counting fallback beyond 8192: cells 0 (9000) and 9 (8193) differ there (fused form: cell 0 = 8193);
  * the 128-entry chunk loop of bev_sum_vec_kernel (`c0`, `clen`, `maxlen`, `cmax`; short neighbours must add nothing in
    later chunks): at C = 80, 4, 128, 256 a wave holds 9000 | 100 | 0 (| 128) members, so a short cell summed again per
    chunk, or a long one cut at its neighbour's length, differs from the oracle in those assertions;
  * the running base of scan_sums: test_scan_beyond_one_chunk's comparison fails for every cell id >= 2,097,152."""
import ctypes

import numpy as np
import pytest
import torch

import bevpool_cases as cases

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CMAX = 260


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _assert_bits(got, ref, what):
    """int32-view equality of two [B, nx0, nx1, nz*C] maps; the message names the first cells that differ."""
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    same = got.view(np.int32) == ref.view(np.int32)
    if not same.all():
        nz = cases.NX[2] if got.shape[1:3] == cases.NX[:2] else 1
        C = got.shape[-1] // nz
        bad = np.argwhere(~same.reshape(got.shape[0], -1, C).all(-1))
        raise AssertionError(f"{what}: {len(bad)} cells differ from the reference, first (sample, cell id): {bad[:8].tolist()}")


@pytest.fixture(scope="module")
def regime_inputs(oracle):
    """geom + one [P, 260] feature matrix whose leading columns serve every C, and the oracle's result per C (computed once)."""
    geom = cases.regimes_geom()
    cases.assert_counts(geom, cases.REGIME_COUNTS)
    x = np.random.default_rng(50).normal(size=(geom.shape[0], CMAX)).astype(np.float32)
    refs = {}

    def ref(C):
        if C not in refs:
            refs[C] = oracle.bev_pool(np.ascontiguousarray(x[:, :C]), geom, cases.B, cases.grid_lo(), cases.DX, cases.NX)
            assert np.abs(refs[C]).sum() > 0
        return refs[C]
    return geom, x, ref


@pytest.mark.parametrize("C", [80, 4, 128, 256, 6, 260])   # float4 kernel at 3 / 4 / 2 / 1 cells per wave; generic kernel (6, 260)
def test_materialised_pool_every_regime(regime_inputs, C):
    """al3d_bev_pool_f32 on the regime input == oracle bit for bit, and twice the same.  Catches a wrong order or a lost /
    repeated member in any of the three list regimes and in the chunk loop (see the module docstring for which cells)."""
    from al3d.models.bevfusion_camera import bev_pool
    geom, x, ref = regime_inputs
    xd, gd = _t(x[:, :C]), _t(geom)
    got = bev_pool(xd, gd, cases.B, cases.DX, cases.BX, cases.NX)
    got2 = bev_pool(xd, gd, cases.B, cases.DX, cases.BX, cases.NX)
    assert got.shape == (cases.B, 24, 20, 2 * C)
    _assert_bits(got, ref(C), f"materialised C={C}")
    assert torch.equal(got, got2)                                           # run-to-run bitwise


def test_materialised_pool_misaligned_x_takes_the_generic_kernel(regime_inputs):
    """x as a contiguous view that starts one float into its storage: (x | out) & 15 != 0, which bev_pool_apply routes to
    bev_sum_kernel although C % 4 == 0.  Same bits as the aligned run (float4 kernel) and as the oracle -- which of the two
    kernels ran is not visible in the result; what is pinned is that neither alignment changes a bit."""
    from al3d.models.bevfusion_camera import bev_pool
    geom, x, ref = regime_inputs
    C, P = 80, geom.shape[0]
    buf = torch.empty(P * C + 1, dtype=torch.float32, device=DEV)
    xm = buf[1:].view(P, C)
    xm.copy_(_t(x[:, :C]))
    assert xm.is_contiguous() and xm.data_ptr() % 16 == 4
    gd = _t(geom)
    got = bev_pool(xm, gd, cases.B, cases.DX, cases.BX, cases.NX)
    aligned = bev_pool(_t(x[:, :C]), gd, cases.B, cases.DX, cases.BX, cases.NX)
    _assert_bits(got, ref(C), "misaligned x, C=80")
    assert torch.equal(got, aligned)


def _plan(geom_d, P, B):
    from al3d import lib
    ncell = B * int(np.prod(cases.NX))
    ws = torch.empty(lib.load().al3d_bev_pool_workspace_bytes(P, ncell), dtype=torch.uint8, device=DEV)
    f3, i3 = ctypes.c_float * 3, ctypes.c_int * 3
    lib.call("al3d_bev_pool_plan", geom_d.data_ptr(), P, B, f3(*cases.grid_lo().tolist()), f3(*cases.DX), i3(*cases.NX),
             ws.data_ptr(), torch.cuda.current_stream().cuda_stream)
    return ws


def _apply(ws, depth_d, ctx_d, B):
    from al3d import lib
    BN, D, fH, fW = depth_d.shape
    C = ctx_d.shape[-1]
    out = torch.empty((B, cases.NX[0], cases.NX[1], cases.NX[2] * C), dtype=torch.float32, device=DEV)
    lib.call("al3d_bev_pool_lss_apply_f32", depth_d.data_ptr(), ctx_d.data_ptr(), BN, D, fH, fW, C, B,
             (ctypes.c_int * 3)(*cases.NX), ws.data_ptr(), out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    return out


@pytest.mark.parametrize("C", [80, 6])                      # bev_sum_vec_kernel<1> (three cells per wave), bev_sum_kernel<1>
def test_fused_lss_pool_every_regime(oracle, C):
    """The fused Lift-Splat form -- what production runs -- with lists of 8193, 8192, 129, 128, 127, 1 and 0 members and a
    long | short | empty wave (asserted on the input first): == oracle.bev_pool(depth=), == pooling the materialised
    product, and through al3d_bev_pool_plan + al3d_bev_pool_lss_apply_f32 directly with ONE plan applied to two different
    (depth, ctx) pairs in turn, each == the oracle (applying does not consume the plan).  A wrong member order, a lost
    member or a wrong (bn, pixel) decomposition of a member index in any regime fails the first comparison."""
    from al3d.models.bevfusion_camera import bev_pool
    B, N, D, fH, fW = cases.LSS_SHAPE
    geom = cases.lss_geom()
    n = cases.assert_counts(geom, cases.LSS_COUNTS)
    assert n[0, 0] > 8192 and n[0, 6] == 8192 and (n[0, 3], n[0, 4]) == (128, 129) and (n[0, 1], n[0, 2]) == (100, 0)
    rng = np.random.default_rng(70 + C)
    gd = _t(geom)
    ws = _plan(gd, geom.shape[0], B)
    for turn in range(2):
        depth = rng.uniform(0, 1, (B * N, D, fH, fW)).astype(np.float32)
        ctx = rng.normal(size=(B * N, fH, fW, C)).astype(np.float32)
        ref = oracle.bev_pool(ctx.reshape(-1, C), geom, B, cases.grid_lo(), cases.DX, cases.NX, depth=depth.reshape(-1), D=D,
                              fHW=fH * fW)
        assert np.abs(ref).sum() > 0
        dd, cd = _t(depth), _t(ctx)
        _assert_bits(_apply(ws, dd, cd, B), ref, f"plan + apply, turn {turn}, C={C}")
        if turn == 0:
            _assert_bits(bev_pool(cd, gd, B, cases.DX, cases.BX, cases.NX, depth=dd), ref, f"fused one-shot C={C}")
            mat = bev_pool(_t((depth[..., None] * ctx[:, None]).reshape(-1, C)), gd, B, cases.DX, cases.BX, cases.NX)
            _assert_bits(mat, ref, f"materialised product C={C}")           # depth_lss.py:93


@pytest.mark.parametrize("C", [80, 5])
def test_cell_boundaries(oracle, C):
    """bev_axis_cell at its edges, per axis: t = (g - lo) / dx exactly 0, in (-1, 0) (kept as cell 0: .long() truncates),
    exactly -1, nx - 2^-k, exactly nx, NaN, +-inf, +-1e30; the first and last cell of each sample; kept points at the last
    index of sample 0 and the first of sample 1.  Against the oracle AND the torch statement of the reference, so the check
    does not rest on the oracle alone."""
    from al3d.models.bevfusion_camera import bev_pool
    geom, kept = cases.boundary_geom()
    assert cases.cell_counts(geom, cases.B).sum() == kept
    x = np.random.default_rng(80 + C).normal(size=(geom.shape[0], C)).astype(np.float32)
    ref = oracle.bev_pool(x, geom, cases.B, cases.grid_lo(), cases.DX, cases.NX)
    stmt = cases.torch_bev_pool(x, geom, cases.B, cases.DX, cases.BX, cases.NX).numpy()
    got = bev_pool(_t(x), _t(geom), cases.B, cases.DX, cases.BX, cases.NX).cpu().numpy()
    _assert_bits(got, ref, f"boundaries C={C}")
    assert np.array_equal(cases.as_reference_layout(got).view(np.int32), stmt.view(np.int32))
    assert np.count_nonzero(np.abs(got).reshape(-1, C).sum(-1)) == np.count_nonzero(cases.cell_counts(geom, cases.B))


def test_scan_beyond_one_chunk(oracle):
    """scan_sums walks the block sums of the shared exclusive scan in 1,024-wide chunks with a running base; a second
    chunk exists only beyond 1,024 x 2,048 = 2,097,152 entries.  B = 1, nx = (1100, 1000, 2) gives 2,200,001 entries: a
    grid just past the smallest that reaches the second chunk (the only other user at that size is the full-size
    voxelizer).  60,000 uniform points, C = 4, == oracle; points in cells with id >= 2,097,152 are asserted to exist: with
    a wrong running base their lists start at the wrong offset and those cells (or the ones they overwrite) differ."""
    from al3d.models.bevfusion_camera import bev_pool
    nx, dx = (1100, 1000, 2), (0.1, 0.1, 4.0)
    bx = (-54.95, -49.95, -2.0)
    lo = cases.grid_lo(dx, bx)                                              # (-55, -50, -4) to float32 rounding
    assert np.allclose(lo, [-55.0, -50.0, -4.0], atol=1e-5) and int(np.prod(nx)) + 1 > 1024 * 2048
    rng = np.random.default_rng(90)
    P, C = 60000, 4
    geom = np.stack([rng.uniform(-55, 55, P), rng.uniform(-50, 50, P), rng.uniform(-4, 4, P)], 1).astype(np.float32)
    n = cases.cell_counts(geom, 1, nx, dx, bx)[0]
    assert n[1024 * 2048:].sum() > 1000 and n[:1024 * 2048].sum() > 1000 and np.count_nonzero(n) > 40000
    x = rng.normal(size=(P, C)).astype(np.float32)
    ref = oracle.bev_pool(x, geom, 1, lo, dx, nx)
    got = bev_pool(_t(x), _t(geom), 1, dx, bx, nx).cpu().numpy()
    same = (got.view(np.int32) == ref.view(np.int32)).reshape(-1, C).all(-1)
    assert same.all(), (f"{int((~same).sum())} cells differ, first ids {np.flatnonzero(~same)[:8].tolist()} "
                        f"(second scan chunk starts at cell {1024 * 2048})")
    assert np.count_nonzero(np.abs(ref).reshape(-1, C).sum(-1)) == np.count_nonzero(n)
