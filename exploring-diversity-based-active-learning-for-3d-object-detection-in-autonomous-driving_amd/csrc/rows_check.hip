// Per-row range check of f16x3 sweep embeddings (AL3D_MATH=auto).
//
// Replaces, per batch and on the device, what sweep.py's _check_range does once per sweep on the gathered
// pool: a row whose [cols] values hold an inf or a NaN is a frame whose activations left the f16x3 range
// (every f16x3 producer lets such a value through as inf/NaN, and the lidar detectors' GAP embedding reads
// everything their head reads).  The sweep copies the flags to the host behind the batch's completion event
// and re-runs only the batches that tripped, under bf16x6.
//
// One wave64 per row, float4 loads where the rows are 16-byte aligned, a wave-level OR (ballot).  The test is
// on the exponent bits, not isfinite(), so that no finite-math flag can fold it away.
#include "al3d_common.h"

#define ROWS_PER_BLOCK 4

__device__ __forceinline__ bool nonfinite_bits(float v)
{
    return (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u;
}

template <bool VEC>
__global__ __launch_bounds__(AL3D_WAVE * ROWS_PER_BLOCK) void rows_nonfinite_kernel(
    const float* __restrict__ x, int rows, int cols, int64_t ld, uint8_t* __restrict__ flags)
{
    const int lane = threadIdx.x & (AL3D_WAVE - 1);
    const int r = blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6);
    if (r >= rows) return;                          // whole waves leave together: r is wave-uniform
    const float* row = x + (int64_t)r * ld;
    bool bad = false;
    int c0 = 0;
    if (VEC) {
        const int c4 = cols >> 2;
        const float4* row4 = reinterpret_cast<const float4*>(row);
        for (int i = lane; i < c4; i += AL3D_WAVE) {
            const float4 v = row4[i];
            bad |= nonfinite_bits(v.x) | nonfinite_bits(v.y) | nonfinite_bits(v.z) | nonfinite_bits(v.w);
        }
        c0 = c4 << 2;
    }
    for (int c = c0 + lane; c < cols; c += AL3D_WAVE) bad |= nonfinite_bits(row[c]);
    const unsigned long long any = __ballot(bad);
    if (lane == 0) flags[r] = any ? 1 : 0;
}

extern "C" int al3d_rows_nonfinite_u8(const float* x, int rows, int cols, int ld, uint8_t* flags, void* stream)
{
    AL3D_REQUIRE(rows >= 0 && cols >= 1 && ld >= cols, "al3d_rows_nonfinite_u8: bad sizes (rows %d, cols %d, ld %d)",
                 rows, cols, ld);
    if (rows == 0) return AL3D_OK;
    AL3D_REQUIRE(x && flags, "al3d_rows_nonfinite_u8: null pointer");
    const dim3 grid((unsigned)al3d_cdiv(rows, ROWS_PER_BLOCK)), block(AL3D_WAVE * ROWS_PER_BLOCK);
    if (((uintptr_t)x & 15) == 0 && (ld & 3) == 0) {
        hipLaunchKernelGGL(rows_nonfinite_kernel<true>, grid, block, 0, (hipStream_t)stream, x, rows, cols,
                           (int64_t)ld, flags);
    } else {
        hipLaunchKernelGGL(rows_nonfinite_kernel<false>, grid, block, 0, (hipStream_t)stream, x, rows, cols,
                           (int64_t)ld, flags);
    }
    AL3D_CHECK_LAUNCH("rows_nonfinite_kernel");
    return AL3D_OK;
}
