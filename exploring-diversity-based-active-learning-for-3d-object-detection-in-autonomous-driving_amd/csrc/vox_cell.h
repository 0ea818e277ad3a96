// Internal (not part of the C ABI): the point -> cell arithmetic and the point -> frame search shared by the hard
// voxelizer (voxelize.hip) and the dynamic one (voxelize_dyn.hip).  Units that include this are built with
// -ffp-contract=off: the float32 subtract/divide/floor must round like numpy.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

struct VoxCfg {
    float min_x, min_y, min_z, vs_x, vs_y, vs_z;
    int gx, gy, gz;         // grid size (x, y, z)
    int max_points, max_voxels, nfeat;
};

__device__ __forceinline__ int64_t vox_cell(const float* __restrict__ p, const VoxCfg& c)
{
    const float fx = floorf((p[0] - c.min_x) / c.vs_x);
    const float fy = floorf((p[1] - c.min_y) / c.vs_y);
    const float fz = floorf((p[2] - c.min_z) / c.vs_z);
    if (!(fx >= 0.f && fx < (float)c.gx && fy >= 0.f && fy < (float)c.gy && fz >= 0.f && fz < (float)c.gz))
        return -1;
    return ((int64_t)(int)fz * c.gy + (int)fy) * c.gx + (int)fx;
}

__device__ __forceinline__ int frame_of(const int64_t* __restrict__ off, int B, int64_t i)
{
    int lo = 0, hi = B;  // largest b with off[b] <= i
    while (hi - lo > 1) { int mid = (lo + hi) >> 1; if (off[mid] <= i) lo = mid; else hi = mid; }
    return lo;
}

// frame_of for a point pass with one point per lane, consecutive in the wave: the frame of the wave's FIRST point by a
// wave-uniform search (scalar loads), then a step forward for the lanes beyond a frame boundary -- a handful of dependent
// vector loads per point otherwise.  Lanes may call it divergently: the first index is derived, not exchanged.
__device__ __forceinline__ int frame_of_wave(const int64_t* __restrict__ off, int B, int64_t i)
{
    const int64_t iw = i - (threadIdx.x & 63);
    const int64_t i0 = ((int64_t)__builtin_amdgcn_readfirstlane((int)(iw >> 32)) << 32) |
                       (unsigned)__builtin_amdgcn_readfirstlane((int)iw);
    int b = frame_of(off, B, i0);
    while (b + 1 < B && off[b + 1] <= i) ++b;
    return b;
}
