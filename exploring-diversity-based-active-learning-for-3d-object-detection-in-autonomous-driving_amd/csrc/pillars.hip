// PointPillars pillar feature net + scatter (fp32 on the VALU, deterministic, no atomics).
//
// Replaces PillarFeatureNet.forward + PFNLayer.forward (det3d/models/readers/pillar_encoder.py:17-152,
// bevfusion/mmdet3d/models/backbones/pillar_encoder.py:47-182) and PointPillarsScatter.forward
// (det3d/models/readers/pillar_encoder.py:155-211, bevfusion/.../pillar_encoder.py:185-240).
//
// One wave64 per pillar; the workgroups loop over the pillars (persistent) with the folded weights resident in LDS.
// Per pillar:
//   - slot p < n (n = num_points clipped to P) is decorated [f_0..f_{F-1}, xyz - mean, x - cx, y - cy, (|xyz|)],
//     mean = sum over the n slots / n; cx = x_index * vx + x_offset, cy = y_index * vy + y_offset.
//   - slots p >= n are zero in the reference and stay in both max reductions.  Zero input through a bias-free linear
//     layer gives relu(shift1) in every such slot (and one identical value after layer 2), so one representative row
//     stands for all P - n of them; the max is exact, so the result is the same.
//   - layer 1: h = relu(x . w1 * scale1 + shift1); m1 = max over the rows.  One layer: out = m1.
//   - layer 2: out = max over the rows of relu(([h, m1]) . w2 * scale2 + shift2).
// Lane u holds units u and u + 64.  The output row is one coalesced store of C floats, to rows [M,C] or to the NHWC
// canvas [B,ny,nx,C] at (b, y, x) of coords (b, z, y, x); the canvas is zeroed by a memset first.
#include "al3d_common.h"

struct PillarArgs {
    const float* voxels;     // [M, P, F]
    const int* num_points;   // [M]
    const int* coords;       // [M, 4] (b, z, y, x)
    const float* w1;         // [fin, U1]      (linear.weight transposed)
    const float* s1;         // [U1]           folded BN scale
    const float* b1;         // [U1]           folded BN shift
    const float* w2;         // [2*U1, U2] or null
    const float* s2;
    const float* b2;
    float* out;
    int M, P, F, fin, U1, U2, C, with_distance;
    float vx, vy, x_offset, y_offset;
    int B, ny, nx, canvas;
};

__global__ __launch_bounds__(256) void pillar_net_kernel(PillarArgs a)
{
    extern __shared__ float lds[];
    const int wpb = blockDim.x >> 6, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int fin = a.fin, U1 = a.U1, U2 = a.U2, P = a.P, F = a.F;
    const bool two = a.w2 != nullptr;
    float* w1 = lds;
    float* s1 = w1 + fin * U1;
    float* b1 = s1 + U1;
    float* w2 = b1 + U1;
    float* s2 = w2 + (two ? 2 * U1 * U2 : 0);
    float* b2 = s2 + (two ? U2 : 0);
    float* per = b2 + (two ? U2 : 0);
    const int per_wave = P * fin + (P + 1) * U1 + U1;
    float* xin = per + wave * per_wave;          // [P][fin] decorated slots
    float* h = xin + P * fin;                    // [P+1][U1] layer-1 rows (row n: the padded-slot representative)
    float* m1 = h + (P + 1) * U1;                // [U1]

    for (int i = threadIdx.x; i < fin * U1; i += blockDim.x) w1[i] = a.w1[i];
    for (int i = threadIdx.x; i < U1; i += blockDim.x) { s1[i] = a.s1[i]; b1[i] = a.b1[i]; }
    if (two) {
        for (int i = threadIdx.x; i < 2 * U1 * U2; i += blockDim.x) w2[i] = a.w2[i];
        for (int i = threadIdx.x; i < U2; i += blockDim.x) { s2[i] = a.s2[i]; b2[i] = a.b2[i]; }
    }
    __syncthreads();

    // every wave of the block takes part in every barrier: the loop count is uniform over the block
    for (int64_t base = (int64_t)blockIdx.x * wpb; base < a.M; base += (int64_t)gridDim.x * wpb) {
        const int64_t pil = base + wave;
        const bool live = pil < a.M;
        int n = live ? a.num_points[pil] : 0;
        n = n < 0 ? 0 : (n > P ? P : n);
        // raw slot values (zero past n)
        float raw[16];
#pragma unroll
        for (int f = 0; f < 16; ++f) raw[f] = 0.f;
        if (lane < n) {
            const float* src = a.voxels + (pil * P + lane) * F;
#pragma unroll
            for (int f = 0; f < 16; ++f)
                if (f < F) raw[f] = src[f];
        }
        if (lane < P) { xin[lane * fin + 0] = raw[0]; xin[lane * fin + 1] = raw[1]; xin[lane * fin + 2] = raw[2]; }
        __syncthreads();
        float mx = 0.f, my = 0.f, mz = 0.f;
        for (int p = 0; p < n; ++p) { mx += xin[p * fin]; my += xin[p * fin + 1]; mz += xin[p * fin + 2]; }
        if (n > 0) { const float d = (float)n; mx /= d; my /= d; mz /= d; }
        __syncthreads();
        if (lane < P) {
            float* row = xin + lane * fin;
            if (lane < n) {
                const int xi = a.coords[pil * 4 + 3], yi = a.coords[pil * 4 + 2];
#pragma unroll
                for (int f = 0; f < 16; ++f)
                    if (f < F) row[f] = raw[f];
                row[F + 0] = raw[0] - mx;
                row[F + 1] = raw[1] - my;
                row[F + 2] = raw[2] - mz;
                row[F + 3] = raw[0] - ((float)xi * a.vx + a.x_offset);
                row[F + 4] = raw[1] - ((float)yi * a.vy + a.y_offset);
                if (a.with_distance) row[F + 5] = sqrtf(raw[0] * raw[0] + raw[1] * raw[1] + raw[2] * raw[2]);
            } else {
                for (int k = 0; k < fin; ++k) row[k] = 0.f;
            }
        }
        __syncthreads();
        const int rows = n + (n < P ? 1 : 0);     // the n point rows + one padded-slot representative
        // layer 1
        float* orow = nullptr;
        if (live) {
            if (a.canvas) {
                const int b = a.coords[pil * 4], y = a.coords[pil * 4 + 2], x = a.coords[pil * 4 + 3];
                if (b >= 0 && b < a.B && y >= 0 && y < a.ny && x >= 0 && x < a.nx)
                    orow = a.out + (((int64_t)b * a.ny + y) * a.nx + x) * a.C;
            } else {
                orow = a.out + pil * a.C;
            }
        }
        for (int u = lane; u < U1; u += 64) {
            const float sc = s1[u], sh = b1[u];
            float best = 0.f;                      // every value is a relu output, >= 0
            for (int p = 0; p < n; ++p) {
                float acc = 0.f;
                for (int k = 0; k < fin; ++k) acc = fmaf(xin[p * fin + k], w1[k * U1 + u], acc);
                const float v = fmaxf(fmaf(acc, sc, sh), 0.f);
                h[p * U1 + u] = v;
                best = fmaxf(best, v);
            }
            if (n < P) {
                const float v = fmaxf(sh, 0.f);
                h[n * U1 + u] = v;
                best = fmaxf(best, v);
            }
            m1[u] = best;
            if (!two && orow) orow[u] = best;
        }
        if (two) {
            __syncthreads();
            for (int v = lane; v < U2; v += 64) {
                float c = 0.f;
                for (int u = 0; u < U1; ++u) c = fmaf(m1[u], w2[(U1 + u) * U2 + v], c);
                const float sc = s2[v], sh = b2[v];
                float best = 0.f;
                for (int r = 0; r < rows; ++r) {
                    float acc = 0.f;
                    for (int u = 0; u < U1; ++u) acc = fmaf(h[r * U1 + u], w2[u * U2 + v], acc);
                    best = fmaxf(best, fmaxf(fmaf(acc + c, sc, sh), 0.f));
                }
                if (orow) orow[v] = best;
            }
        }
        __syncthreads();
    }
}

static int pillar_launch(PillarArgs a, void* stream, const char* name)
{
    AL3D_REQUIRE(a.M >= 0 && a.P >= 1 && a.P <= 64 && a.F >= 3 && a.F <= 10,
                 "%s: bad sizes (M %d, P %d, F %d; need 1 <= P <= 64, 3 <= F <= 10)", name, a.M, a.P, a.F);
    AL3D_REQUIRE(a.U1 >= 16 && a.U1 <= 128 && a.U1 % 16 == 0, "%s: layer 1 units %d: need a multiple of 16 in [16, 128]",
                 name, a.U1);
    if (a.w2) {
        AL3D_REQUIRE(a.U2 >= 16 && a.U2 <= 128 && a.U2 % 16 == 0,
                     "%s: layer 2 units %d: need a multiple of 16 in [16, 128]", name, a.U2);
        AL3D_REQUIRE(a.s2 && a.b2, "%s: layer 2 scale/shift missing", name);
    } else {
        a.U2 = 0;
    }
    a.fin = a.F + 5 + (a.with_distance ? 1 : 0);
    a.C = a.w2 ? a.U2 : a.U1;
    AL3D_REQUIRE(a.w1 && a.s1 && a.b1, "%s: null weight pointer", name);
    AL3D_REQUIRE(a.M == 0 || (a.voxels && a.num_points && a.coords && a.out), "%s: null pointer", name);
    const int64_t fixed = (int64_t)a.fin * a.U1 + 2 * a.U1 + (a.w2 ? 2 * a.U1 * a.U2 + 2 * a.U2 : 0);
    const int64_t per_wave = (int64_t)a.P * a.fin + (int64_t)(a.P + 1) * a.U1 + a.U1;
    int wpb = 4;
    while (wpb > 1 && (fixed + wpb * per_wave) * 4 > 64 * 1024) wpb >>= 1;
    const int64_t bytes = (fixed + wpb * per_wave) * 4;
    AL3D_REQUIRE(bytes <= 160 * 1024, "%s: %lld bytes of LDS needed (> 160 KiB)", name, (long long)bytes);
    if (bytes > 64 * 1024 &&
        hipFuncSetAttribute((const void*)pillar_net_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) !=
            hipSuccess)
        return al3d_fail(AL3D_ELAUNCH, "%s: cannot raise the LDS limit", name);
    if (a.canvas &&
        hipMemsetAsync(a.out, 0, (size_t)a.B * a.ny * a.nx * a.C * sizeof(float), (hipStream_t)stream) != hipSuccess)
        return al3d_fail(AL3D_ELAUNCH, "%s: canvas memset failed", name);
    if (a.M == 0) return AL3D_OK;
    const int64_t blocks = al3d_cdiv(a.M, wpb);
    const int grid = (int)(blocks < 4096 ? blocks : 4096);
    hipLaunchKernelGGL(pillar_net_kernel, dim3(grid), dim3(64 * wpb), (size_t)bytes, (hipStream_t)stream, a);
    AL3D_CHECK_LAUNCH("pillar_net_kernel");
    return AL3D_OK;
}

extern "C" int al3d_pillar_net_f32(const float* voxels, const int* num_points, const int* coords, int M, int P, int F,
                                   float vx, float vy, float x_offset, float y_offset, int with_distance,
                                   const float* w1, const float* s1, const float* b1, int U1,
                                   const float* w2, const float* s2, const float* b2, int U2, float* out, void* stream)
{
    PillarArgs a{voxels, num_points, coords, w1, s1, b1, w2, s2, b2, out, M, P, F, 0, U1, U2, 0, with_distance,
                 vx, vy, x_offset, y_offset, 0, 0, 0, 0};
    return pillar_launch(a, stream, "al3d_pillar_net_f32");
}

extern "C" int al3d_pillar_net_scatter_f32(const float* voxels, const int* num_points, const int* coords, int M, int P,
                                           int F, float vx, float vy, float x_offset, float y_offset, int with_distance,
                                           const float* w1, const float* s1, const float* b1, int U1,
                                           const float* w2, const float* s2, const float* b2, int U2,
                                           int B, int ny, int nx, float* canvas, void* stream)
{
    AL3D_REQUIRE(B >= 0 && ny >= 1 && nx >= 1 && canvas, "al3d_pillar_net_scatter_f32: bad canvas (B %d, %d x %d)", B,
                 ny, nx);
    PillarArgs a{voxels, num_points, coords, w1, s1, b1, w2, s2, b2, canvas, M, P, F, 0, U1, U2, 0, with_distance,
                 vx, vy, x_offset, y_offset, B, ny, nx, 1};
    return pillar_launch(a, stream, "al3d_pillar_net_scatter_f32");
}

// PointPillarsScatter alone: rows [M,C] -> zeroed NHWC canvas [B,ny,nx,C]; one wave per row, one coalesced row store.
__global__ __launch_bounds__(256) void pillar_scatter_kernel(const float* __restrict__ rows, const int* __restrict__ coords,
                                                             int M, int C, int B, int ny, int nx, float* __restrict__ canvas)
{
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (r >= M) return;
    const int b = coords[r * 4], y = coords[r * 4 + 2], x = coords[r * 4 + 3];
    if (b < 0 || b >= B || y < 0 || y >= ny || x < 0 || x >= nx) return;
    float* dst = canvas + (((int64_t)b * ny + y) * nx + x) * C;
    for (int c = lane; c < C; c += 64) dst[c] = rows[r * C + c];
}

extern "C" int al3d_pillar_scatter_nhwc_f32(const float* rows, const int* coords, int M, int C, int B, int ny, int nx,
                                            float* canvas, void* stream)
{
    AL3D_REQUIRE(M >= 0 && C >= 1 && B >= 0 && ny >= 1 && nx >= 1 && canvas,
                 "al3d_pillar_scatter_nhwc_f32: bad sizes (M %d, C %d, B %d, %d x %d)", M, C, B, ny, nx);
    if (hipMemsetAsync(canvas, 0, (size_t)B * ny * nx * C * sizeof(float), (hipStream_t)stream) != hipSuccess)
        return al3d_fail(AL3D_ELAUNCH, "al3d_pillar_scatter_nhwc_f32: canvas memset failed");
    if (M == 0) return AL3D_OK;
    AL3D_REQUIRE(rows && coords, "al3d_pillar_scatter_nhwc_f32: null pointer");
    hipLaunchKernelGGL(pillar_scatter_kernel, dim3((unsigned)al3d_cdiv(M, 4)), dim3(256), 0, (hipStream_t)stream, rows,
                       coords, M, C, B, ny, nx, canvas);
    AL3D_CHECK_LAUNCH("pillar_scatter_kernel");
    return AL3D_OK;
}
