"""GPU suite: the device-wide exclusive scan (csrc/scan_kernels.hip) through its exported entry, exact against numpy's
int64 cumulative sum.  The sizes sit on each side of a wave (64), of one workgroup's 2048 items, and of the 1024 block sums
one pass of the middle kernel takes (2048 * 1024 items); every case also runs in place, the form the dynamic voxelizer
uses, and inside guard bytes."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ITEMS, CHUNK = 2048, 1024
SIZES = [1, 2, 63, 64, 65, 2047, 2048, 2049, 4096, ITEMS * CHUNK - 1, ITEMS * CHUNK, ITEMS * CHUNK + 1,
         2 * ITEMS * CHUNK + 5]
PATTERNS = ["random", "zeros", "ones", "last"]
GUARD = 1024                     # bytes of pattern on each side of the workspace
FILL = 0x5A


def values(n, pattern):
    if pattern == "random":
        return np.random.default_rng(n).integers(0, 500, n).astype(np.int32)
    if pattern == "zeros":
        return np.zeros(n, np.int32)
    if pattern == "ones":
        return np.ones(n, np.int32)
    v = np.zeros(n, np.int32)
    v[-1] = 7
    return v


def exclusive(v):
    inc = np.cumsum(v.astype(np.int64))
    assert inc[-1] < 2 ** 31
    return (inc - v).astype(np.int32)


def run_scan(v, in_place):
    """-> (result, input buffer afterwards); checks the guard bytes round the workspace and behind the output."""
    from al3d import lib
    n = len(v)
    nbytes = lib.load().al3d_scan_exclusive_workspace_bytes(n)
    assert nbytes >= 4 * (-(-n // ITEMS))
    raw = torch.full((nbytes + 2 * GUARD,), FILL, dtype=torch.uint8, device=DEV)
    src = torch.from_numpy(v).to(DEV)
    buf = torch.full((n + 64,), -77, dtype=torch.int32, device=DEV)
    if in_place:
        buf[:n] = src
        inp = buf
    else:
        inp = src
    lib.call("al3d_scan_exclusive_i32", inp.data_ptr(), buf.data_ptr(), n, raw.data_ptr() + GUARD,
             torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert bool((raw[:GUARD] == FILL).all()) and bool((raw[GUARD + nbytes:] == FILL).all()), "wrote outside the workspace"
    assert bool((buf[n:] == -77).all()), "wrote past out[n]"
    return buf[:n].cpu().numpy(), src.cpu().numpy()


@pytest.mark.parametrize("n", SIZES)
def test_exclusive_scan_equals_cumsum(n):
    for pattern in PATTERNS:
        v = values(n, pattern)
        want = exclusive(v)
        got, src = run_scan(v, in_place=False)
        assert np.array_equal(src, v), (pattern, "the input changed")
        assert np.array_equal(got, want), (pattern, "separate buffers")
        got, _ = run_scan(v, in_place=True)
        assert np.array_equal(got, want), (pattern, "in place")


def test_workspace_size_and_the_empty_scan():
    from al3d import lib
    so = lib.load()
    for n in (0, 1, ITEMS, ITEMS + 1, ITEMS * CHUNK + 1):
        nb = so.al3d_scan_exclusive_workspace_bytes(n)
        assert nb >= 4 * (-(-n // ITEMS))                 # one int per workgroup's 2048 items at the least
    out = torch.full((8,), 3, dtype=torch.int32, device=DEV)
    lib.call("al3d_scan_exclusive_i32", out.data_ptr(), out.data_ptr(), 0, None, None)
    torch.cuda.synchronize()
    assert out.tolist() == [3] * 8
