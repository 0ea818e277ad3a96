// Dynamic PointPillars pillar feature net: every point of every pillar, no padded slots (fp32 on the VALU).
//
// The net of pillars.hip (PillarFeatureNet.forward + PFNLayer.forward, det3d/models/readers/pillar_encoder.py:17-152,
// bevfusion/mmdet3d/models/backbones/pillar_encoder.py:47-182) on the output of the dynamic voxelizer
// (voxelize_dyn.hip): points [npts,F] in any order, point2voxel [npts] (row of the point's pillar or -1), the pillar
// means and the pillar coordinates.  Pillars hold anywhere from one point to several thousand, so the work is parallel
// over POINTS and pooled by pillar:
//   - lanes are output units (lane u holds units u and u + 64); a wave walks a contiguous chunk of points, PD_T at a time.
//     The step's decoration is one pass (lane 16 t + k forms input k of point t); inputs and h go from lane to lane by
//     readlane; the layer-1 columns sit in registers, the upper half of w2 (the rows that read h) in LDS.
//   - every expression is written as pillars.hip writes it (decoration :91-96, chains :118-120 and :135-142), so a pillar
//     without padded slots gets the hard kernel's bits.
//   - pooling: each lane keeps a running max while consecutive points share a pillar and flushes when the pillar changes:
//     a signed-integer atomic max on the value's bit pattern, after a plain read that skips it when the destination
//     already holds as much.  Every pooled value is a relu output and the destination starts at +0, so zeros (and -0,
//     negative as an integer) never issue an atomic.  A max does not depend on arrival order: the result is the same
//     bits from run to run, for every point order and every launch shape.
//   - two layers: launch 1 pools m1 [M,U1] into the workspace, a per-pillar launch forms c = m1 . w2[U1:] (the half of
//     layer 2 every point of the pillar shares), launch 2 recomputes h per point and pools the output.  Nothing of size
//     [npts, U1] is stored; there is no grid-wide wait.
// The one deliberate difference to pillars.hip: there is no padded-slot representative row.  A hard pillar with
// n < P points also pools relu(shift1) (and its layer-2 image); here only points count.
#include "al3d_common.h"

#define PD_T 4              // points per step of a wave: 16 lanes decorate one point (at most 16 inputs)
static_assert(PD_T * 16 == 64, "one wave decorates PD_T points of 16 inputs each");
#define PD_CHUNK 64         // points per wave chunk (default)
#define PD_BLOCKS 2048      // most blocks of a point launch (default)

struct PdGeom {
    int64_t npts, M;
    int F, fin, U1, U2, C, with_distance, mean_ld;
    float vx, vy, x_offset, y_offset;
    int B, ny, nx, canvas, chunk;
};

__device__ __forceinline__ float pd_lane(float v, int l)
{
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}

// destination row of pillar r: rows [M,C], or the NHWC cell (b, y, x); null when the cell lies outside the canvas
__device__ __forceinline__ float* pd_row(const PdGeom& g, const int* __restrict__ coords, float* dst, int64_t r)
{
    if (!g.canvas) return dst + r * g.C;
    const int b = coords[r * 4], y = coords[r * 4 + 2], x = coords[r * 4 + 3];
    if (b < 0 || b >= g.B || y < 0 || y >= g.ny || x < 0 || x >= g.nx) return nullptr;
    return dst + (((int64_t)b * g.ny + y) * g.nx + x) * g.C;
}

// L2 = false: pool layer 1 into dst (rows of U1: the workspace m1, or the output of a one-layer net).
// L2 = true : recompute layer 1, run layer 2 with the pillar's c = cvec[r] and pool into dst (rows of U2).
// WIDE2: layer 2 has more than 64 units (the lanes' second unit exists); otherwise that half of the work is not compiled in.
template <bool L2, bool WIDE2>
__global__ __launch_bounds__(256) void pd_points_kernel(
    PdGeom g, const float* __restrict__ points, const int* __restrict__ p2v, const float* __restrict__ mean,
    const int* __restrict__ coords, const float* __restrict__ w1, const float* __restrict__ s1,
    const float* __restrict__ b1, const float* __restrict__ w2, const float* __restrict__ s2,
    const float* __restrict__ b2, const float* __restrict__ cvec, float* dst, int* status)
{
    extern __shared__ float w2s[];                          // L2: w2 rows 0..U1-1, [U1][U2]
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int fin = g.fin, U1 = g.U1, U2 = g.U2, F = g.F;
    const int u0 = lane, u1 = lane + 64;
    const bool ok0 = u0 < U1, ok1 = u1 < U1;
    float wa[16], wb[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        wa[k] = (k < fin && ok0) ? w1[k * U1 + u0] : 0.f;
        wb[k] = (k < fin && ok1) ? w1[k * U1 + u1] : 0.f;
    }
    const float sa = ok0 ? s1[u0] : 0.f, ba = ok0 ? b1[u0] : 0.f;
    const float sb = ok1 ? s1[u1] : 0.f, bb = ok1 ? b1[u1] : 0.f;
    // the lane's pooled units: layer 2's when L2
    const int UO = L2 ? U2 : U1;
    const bool oko0 = lane < UO, oko1 = lane + 64 < UO;
    const int v0 = oko0 ? lane : 0, v1 = oko1 ? lane + 64 : 0;        // clamped: addresses stay inside the arrays
    float s2a = 0.f, b2a = 0.f, s2b = 0.f, b2b = 0.f;
    if (L2) {
        for (int i = threadIdx.x; i < U1 * U2; i += blockDim.x) w2s[i] = w2[i];
        s2a = s2[v0]; b2a = b2[v0]; s2b = s2[v1]; b2b = b2[v1];
        __syncthreads();
    }

    const int64_t nchunks = (g.npts + g.chunk - 1) / g.chunk;
    int bad = 0;
    // no block barrier below: the waves of a block may run different numbers of chunks
    for (int64_t c = (int64_t)blockIdx.x * 4 + wave; c < nchunks; c += (int64_t)gridDim.x * 4) {
        const int64_t i0 = c * g.chunk, i1 = i0 + g.chunk < g.npts ? i0 + g.chunk : g.npts;
        int64_t cur = -1;
        float best0 = 0.f, best1 = 0.f;                   // every value is a relu output, >= 0
        auto flush = [&]() {
            if (cur < 0) return;
            float* row = pd_row(g, coords, dst, cur);
            if (row) {
                int* irow = (int*)row;
                // signed compare: -0.f is negative, +0.f is what the destination starts with
                const int q0 = __float_as_int(best0), q1 = __float_as_int(best1);
                if (oko0 && q0 > 0 && q0 > irow[lane]) atomicMax(irow + lane, q0);
                if (oko1 && q1 > 0 && q1 > irow[lane + 64]) atomicMax(irow + lane + 64, q1);
            }
        };
        // decoration of the step at i: lane 16 t + k forms input k of point i + t (one pass for the step's PD_T points); the
        // inputs then go to every lane by readlane.  Each expression as pillars.hip:91-96 writes it
        auto decorate = [&](int64_t i, float& xv, int& rl) {
            const int tl = lane >> 4, kl = lane & 15;
            const bool in = i + tl < i1;
            rl = in ? p2v[i + tl] : -1;
            const bool oob = rl < -1 || (int64_t)rl >= g.M;
            if (oob) rl = -1;                                           // never index with it
            if (__ballot(oob) != 0ull) bad = 1;
            const int64_t rr = rl < 0 ? 0 : rl;                         // M > 0 here: row 0 exists
            const float* src = points + (in ? i + tl : i0) * F;
            const float r0 = src[0], r1 = src[1], r2 = src[2];
            const int j = kl - F;
            xv = 0.f;
            if (kl < F) {
                xv = src[kl];
            } else if (j < 3) {
                xv = (j == 0 ? r0 : (j == 1 ? r1 : r2)) - mean[rr * g.mean_ld + j];
            } else if (j == 3) {
                xv = r0 - ((float)coords[rr * 4 + 3] * g.vx + g.x_offset);
            } else if (j == 4) {
                xv = r1 - ((float)coords[rr * 4 + 2] * g.vy + g.y_offset);
            } else if (j == 5 && g.with_distance) {
                xv = sqrtf(r0 * r0 + r1 * r1 + r2 * r2);
            }
        };
        float xnext;
        int rnext;
        decorate(i0, xnext, rnext);
        for (int64_t i = i0; i < i1; i += PD_T) {
            int64_t row_of[PD_T];
            float h0[PD_T], h1[PD_T];
            const float xv = xnext;
            const int rl = rnext;
            if (i + PD_T < i1) decorate(i + PD_T, xnext, rnext);       // the next step's loads fly during this step's layers
#pragma unroll
            for (int t = 0; t < PD_T; ++t) {
                row_of[t] = __builtin_amdgcn_readlane(rl, 16 * t);
                float a0 = 0.f, a1 = 0.f;
#pragma unroll
                for (int k = 0; k < 8; ++k) {                           // fin >= 8
                    const float xk = pd_lane(xv, 16 * t + k);
                    a0 = fmaf(xk, wa[k], a0);
                    a1 = fmaf(xk, wb[k], a1);
                }
#pragma unroll
                for (int k = 8; k < 16; ++k)
                    if (k < fin) {
                        const float xk = pd_lane(xv, 16 * t + k);
                        a0 = fmaf(xk, wa[k], a0);
                        a1 = fmaf(xk, wb[k], a1);
                    }
                h0[t] = fmaxf(fmaf(a0, sa, ba), 0.f);
                h1[t] = fmaxf(fmaf(a1, sb, bb), 0.f);
            }
            float o0[PD_T], o1[PD_T];
            if (L2) {
                float e0[PD_T], e1[PD_T];
#pragma unroll
                for (int t = 0; t < PD_T; ++t) { e0[t] = 0.f; e1[t] = 0.f; }
                const int ua = U1 < 64 ? U1 : 64;
                for (int u = 0; u < ua; ++u) {
                    const float wv0 = w2s[u * U2 + v0], wv1 = WIDE2 ? w2s[u * U2 + v1] : 0.f;
#pragma unroll
                    for (int t = 0; t < PD_T; ++t) {
                        const float hv = pd_lane(h0[t], u);
                        e0[t] = fmaf(hv, wv0, e0[t]);
                        if (WIDE2) e1[t] = fmaf(hv, wv1, e1[t]);
                    }
                }
                for (int u = 64; u < U1; ++u) {
                    const float wv0 = w2s[u * U2 + v0], wv1 = WIDE2 ? w2s[u * U2 + v1] : 0.f;
#pragma unroll
                    for (int t = 0; t < PD_T; ++t) {
                        const float hv = pd_lane(h1[t], u - 64);
                        e0[t] = fmaf(hv, wv0, e0[t]);
                        if (WIDE2) e1[t] = fmaf(hv, wv1, e1[t]);
                    }
                }
#pragma unroll
                for (int t = 0; t < PD_T; ++t) {
                    const int64_t rr = row_of[t] < 0 ? 0 : row_of[t];
                    const float c0 = cvec[rr * U2 + v0];
                    o0[t] = fmaxf(fmaf(e0[t] + c0, s2a, b2a), 0.f);
                    o1[t] = WIDE2 ? fmaxf(fmaf(e1[t] + cvec[rr * U2 + v1], s2b, b2b), 0.f) : 0.f;
                }
            } else {
#pragma unroll
                for (int t = 0; t < PD_T; ++t) { o0[t] = h0[t]; o1[t] = h1[t]; }
            }
#pragma unroll
            for (int t = 0; t < PD_T; ++t) {
                if (row_of[t] < 0) continue;                 // wave-uniform
                if (row_of[t] != cur) { flush(); cur = row_of[t]; best0 = 0.f; best1 = 0.f; }
                best0 = fmaxf(best0, o0[t]);
                best1 = fmaxf(best1, o1[t]);
            }
        }
        flush();
    }
    if (bad && lane == 0) atomicOr(status, 1);
}

// c[r][v] = chain over u of m1[r][u] * w2[(U1 + u) * U2 + v] (pillars.hip:136); one wave per pillar, w2's lower half in LDS
__global__ __launch_bounds__(256) void pd_context_kernel(int64_t M, int U1, int U2, const float* __restrict__ m1,
                                                         const float* __restrict__ w2, float* __restrict__ cvec)
{
    extern __shared__ float w2s[];                          // [U1][U2]: rows U1..2*U1-1 of w2
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (int i = threadIdx.x; i < U1 * U2; i += blockDim.x) w2s[i] = w2[U1 * U2 + i];
    __syncthreads();
    const bool ok0 = lane < U2, ok1 = lane + 64 < U2;
    const int v0 = ok0 ? lane : 0, v1 = ok1 ? lane + 64 : 0;
    for (int64_t r = (int64_t)blockIdx.x * 4 + wave; r < M; r += (int64_t)gridDim.x * 4) {
        const float ma = lane < U1 ? m1[r * U1 + lane] : 0.f;
        const float mb = lane + 64 < U1 ? m1[r * U1 + lane + 64] : 0.f;
        float c0 = 0.f, c1 = 0.f;
        const int ua = U1 < 64 ? U1 : 64;
        for (int u = 0; u < ua; ++u) {
            const float mv = pd_lane(ma, u);
            c0 = fmaf(mv, w2s[u * U2 + v0], c0);
            c1 = fmaf(mv, w2s[u * U2 + v1], c1);
        }
        for (int u = 64; u < U1; ++u) {
            const float mv = pd_lane(mb, u - 64);
            c0 = fmaf(mv, w2s[u * U2 + v0], c0);
            c1 = fmaf(mv, w2s[u * U2 + v1], c1);
        }
        if (ok0) cvec[r * U2 + lane] = c0;
        if (ok1) cvec[r * U2 + lane + 64] = c1;
    }
}

// m1 [M,U1] then c [M,128] (U2 <= 128): the workspace of a two-layer net; one layer needs none
extern "C" int64_t al3d_pillar_net_dynamic_workspace_bytes(int64_t M, int U1, int two_layers)
{
    if (M <= 0 || U1 <= 0 || !two_layers) return 0;
    return M * ((int64_t)U1 + 128) * (int64_t)sizeof(float);
}

extern "C" int al3d_pillar_net_dynamic_launch_f32(
    const float* points, const int* point2voxel, int64_t npts, int F, const float* mean, int mean_ld, const int* coords,
    int64_t M, float vx, float vy, float x_offset, float y_offset, int with_distance, const float* w1, const float* s1,
    const float* b1, int U1, const float* w2, const float* s2, const float* b2, int U2, int B, int ny, int nx, float* out,
    int canvas, void* workspace, int* status, int chunk_points, int max_blocks, void* stream)
{
    const char* name = "al3d_pillar_net_dynamic_f32";
    hipStream_t st = (hipStream_t)stream;
    AL3D_REQUIRE(npts >= 0 && M >= 0 && F >= 3 && F <= 10, "%s: bad sizes (npts %lld, M %lld, F %d; need 3 <= F <= 10)", name,
                 (long long)npts, (long long)M, F);
    AL3D_REQUIRE(U1 >= 16 && U1 <= 128 && U1 % 16 == 0, "%s: layer 1 units %d: need a multiple of 16 in [16, 128]", name, U1);
    if (w2) {
        AL3D_REQUIRE(U2 >= 16 && U2 <= 128 && U2 % 16 == 0, "%s: layer 2 units %d: need a multiple of 16 in [16, 128]", name,
                     U2);
        AL3D_REQUIRE(s2 && b2, "%s: layer 2 scale/shift missing", name);
    } else {
        U2 = 0;
    }
    AL3D_REQUIRE(w1 && s1 && b1, "%s: null weight pointer", name);
    AL3D_REQUIRE(status, "%s: null status pointer", name);
    AL3D_REQUIRE(chunk_points >= 0 && max_blocks >= 0, "%s: bad launch shape (chunk %d, blocks %d)", name, chunk_points,
                 max_blocks);
    const int C = w2 ? U2 : U1;
    if (canvas) {
        AL3D_REQUIRE(B >= 0 && ny >= 1 && nx >= 1 && out, "%s: bad canvas (B %d, %d x %d)", name, B, ny, nx);
        if (hipMemsetAsync(out, 0, (size_t)B * ny * nx * C * sizeof(float), st) != hipSuccess)
            return al3d_fail(AL3D_ELAUNCH, "%s: canvas memset failed", name);
    } else if (M > 0) {
        AL3D_REQUIRE(out, "%s: null output pointer", name);
        if (hipMemsetAsync(out, 0, (size_t)M * C * sizeof(float), st) != hipSuccess)
            return al3d_fail(AL3D_ELAUNCH, "%s: output memset failed", name);
    }
    if (npts == 0 || M == 0) return AL3D_OK;
    AL3D_REQUIRE(points && point2voxel && mean && coords && mean_ld >= 3, "%s: null pointer or mean_ld %d < 3", name,
                 mean_ld);
    AL3D_REQUIRE(!w2 || workspace, "%s: two layers need the workspace", name);

    PdGeom g{};
    g.npts = npts; g.M = M; g.F = F; g.fin = F + 5 + (with_distance ? 1 : 0); g.U1 = U1; g.U2 = U2;
    g.with_distance = with_distance ? 1 : 0; g.mean_ld = mean_ld;
    g.vx = vx; g.vy = vy; g.x_offset = x_offset; g.y_offset = y_offset;
    g.chunk = chunk_points > 0 ? chunk_points : PD_CHUNK;
    const int64_t nchunks = al3d_cdiv(npts, g.chunk);
    const int64_t cap = max_blocks > 0 ? max_blocks : PD_BLOCKS;
    const int64_t want = al3d_cdiv(nchunks, 4);
    const unsigned grid = (unsigned)(want < cap ? want : cap);

    if (!w2) {
        g.C = U1; g.B = B; g.ny = ny; g.nx = nx; g.canvas = canvas ? 1 : 0;
        hipLaunchKernelGGL((pd_points_kernel<false, false>), dim3(grid), dim3(256), 0, st, g, points, point2voxel, mean, coords, w1, s1,
                           b1, nullptr, nullptr, nullptr, nullptr, out, status);
        AL3D_CHECK_LAUNCH("pd_points_kernel<layer 1>");
        return AL3D_OK;
    }
    float* m1 = (float*)workspace;
    float* cvec = m1 + M * U1;
    if (hipMemsetAsync(m1, 0, (size_t)M * U1 * sizeof(float), st) != hipSuccess)
        return al3d_fail(AL3D_ELAUNCH, "%s: workspace memset failed", name);
    PdGeom g1 = g;
    g1.C = U1; g1.canvas = 0;
    hipLaunchKernelGGL((pd_points_kernel<false, false>), dim3(grid), dim3(256), 0, st, g1, points, point2voxel, mean, coords, w1, s1, b1,
                       nullptr, nullptr, nullptr, nullptr, m1, status);
    AL3D_CHECK_LAUNCH("pd_points_kernel<layer 1>");
    const size_t lds = (size_t)U1 * U2 * sizeof(float);    // at most 64 KiB
    const int64_t cblocks = al3d_cdiv(M, 4);
    hipLaunchKernelGGL(pd_context_kernel, dim3((unsigned)(cblocks < 1024 ? cblocks : 1024)), dim3(256), lds, st, M, U1, U2, m1,
                       w2, cvec);
    AL3D_CHECK_LAUNCH("pd_context_kernel");
    g.C = U2; g.B = B; g.ny = ny; g.nx = nx; g.canvas = canvas ? 1 : 0;
    if (U2 > 64)
        hipLaunchKernelGGL((pd_points_kernel<true, true>), dim3(grid), dim3(256), lds, st, g, points, point2voxel, mean, coords,
                           w1, s1, b1, w2, s2, b2, cvec, out, status);
    else
        hipLaunchKernelGGL((pd_points_kernel<true, false>), dim3(grid), dim3(256), lds, st, g, points, point2voxel, mean, coords,
                           w1, s1, b1, w2, s2, b2, cvec, out, status);
    AL3D_CHECK_LAUNCH("pd_points_kernel<layer 2>");
    return AL3D_OK;
}

extern "C" int al3d_pillar_net_dynamic_f32(
    const float* points, const int* point2voxel, int64_t npts, int F, const float* mean, int mean_ld, const int* coords,
    int64_t M, float vx, float vy, float x_offset, float y_offset, int with_distance, const float* w1, const float* s1,
    const float* b1, int U1, const float* w2, const float* s2, const float* b2, int U2, int B, int ny, int nx, float* out,
    int canvas, void* workspace, int* status, void* stream)
{
    return al3d_pillar_net_dynamic_launch_f32(points, point2voxel, npts, F, mean, mean_ld, coords, M, vx, vy, x_offset,
                                              y_offset, with_distance, w1, s1, b1, U1, w2, s2, b2, U2, B, ny, nx, out, canvas,
                                              workspace, status, 0, 0, stream);
}
