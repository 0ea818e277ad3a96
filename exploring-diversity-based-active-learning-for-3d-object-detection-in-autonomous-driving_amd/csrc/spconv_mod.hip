// Index and pooling kernels of the spconv-1.x module surface (al3d.spconv), gfx950.
//
// The convolutions of that surface are the launches of csrc/spconv*.hip; this file holds what the encoder never needed:
//   * a bounds check of a caller's [n, 4] coordinate array (the encoder's coordinates come from our own voxelizer, a
//     module's from anywhere), run before any kernel indexes a grid by them;
//   * SparseMaxPool3d over a tap-major table;
//   * the rulebooks of SparseInverseConv3d (the paired layer's table, inverted) and SparseConvTranspose3d (input i feeds the
//     output cell i*s - p + d_k at tap k), in the output-major form every conv kernel here reads: nbr[k][o] = input row or -1;
//   * a VALU convolution for channel pairs no templated kernel is built for.
// All of it is integer work or f32 comparisons and fixed-order f32 FMA chains: deterministic, no float atomic.  The integer
// atomicOr's below set bits of per-tile tap masks / of a status word (idempotent, order-free).
#include "al3d_common.h"
#include "sp_sites.h"

struct SmDims { int B, D, H, W; };
struct SmGeom { int kd, kh, kw, sd, sh, sw, pd, ph, pw; };

__device__ __forceinline__ int64_t sm_cell(const SmDims& g, int b, int z, int y, int x)
{
    return (((int64_t)b * g.D + z) * g.H + y) * g.W + x;
}

static inline unsigned sm_blocks(int64_t n, int per) { return (unsigned)al3d_cdiv(n > 0 ? n : 1, per); }

// ------------------------------------------------------------------ coordinate check
// bit 0: batch, 1: z, 2: y, 3: x outside its range.  Reads the coordinate rows only.
__global__ void sm_coords_check_kernel(const int* __restrict__ coords, int n, SmDims g, int* __restrict__ status)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int4 c = *reinterpret_cast<const int4*>(coords + 4 * (int64_t)i);
    const int bad = ((unsigned)c.x >= (unsigned)g.B ? 1 : 0) | ((unsigned)c.y >= (unsigned)g.D ? 2 : 0) |
                    ((unsigned)c.z >= (unsigned)g.H ? 4 : 0) | ((unsigned)c.w >= (unsigned)g.W ? 8 : 0);
    if (bad) atomicOr(status, bad);
}

extern "C" int al3d_sp_coords_check(const int* coords, int n, int B, int D, int H, int W, int* status, void* stream)
{
    AL3D_REQUIRE(status && n >= 0 && B >= 1 && D >= 1 && H >= 1 && W >= 1, "al3d_sp_coords_check: bad arguments");
    AL3D_REQUIRE((int64_t)B * D * H * W < (1LL << 31), "al3d_sp_coords_check: B*D*H*W must be below 2^31");
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(status, 0, 4, s) != hipSuccess) return al3d_fail(AL3D_ELAUNCH, "al3d_sp_coords_check: memset failed");
    if (n == 0) return AL3D_OK;
    AL3D_REQUIRE(coords && ((uintptr_t)coords & 15) == 0, "al3d_sp_coords_check: coords must be non-null, 16-byte aligned");
    SmDims g = {B, D, H, W};
    hipLaunchKernelGGL(sm_coords_check_kernel, dim3(sm_blocks(n, 256)), dim3(256), 0, s, coords, n, g, status);
    AL3D_CHECK_LAUNCH("sm_coords_check_kernel");
    return AL3D_OK;
}

// ------------------------------------------------------------------ max pool
// out[o][c] = max over the taps k with nbr[k][o] >= 0 of feats[nbr[k][o]][c]; one thread per (row, V channels): the lanes of
// a row read consecutive addresses of each gathered row, the table entry is the same word for all of them.  `m < v` keeps
// the running value when v is NaN, as the reference's comparison does (pool_ops.h:34); zero_floor starts from the
// reference's zero-initialised output (maxpool.cc:36), else from -inf.
template <int V>
__global__ void sm_maxpool_kernel(const float* __restrict__ feats, const int* __restrict__ nbr, int64_t ld, int K, int C,
                                  int n_out, int zero_floor, float* __restrict__ out)
{
    const int cv = C / V;
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (int64_t)n_out * cv) return;
    const int o = (int)(e / cv), c = (int)(e % cv) * V;
    float m[V];
#pragma unroll
    for (int j = 0; j < V; ++j) m[j] = zero_floor ? 0.f : -__builtin_inff();
    for (int k = 0; k < K; ++k) {
        const int i = nbr[(int64_t)k * ld + o];
        if (i < 0) continue;
        const float* src = feats + (int64_t)i * C + c;
        float v[V];
        if constexpr (V == 4) {
            const float4 t = *reinterpret_cast<const float4*>(src);
            v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
        } else {
            v[0] = src[0];
        }
#pragma unroll
        for (int j = 0; j < V; ++j) if (m[j] < v[j]) m[j] = v[j];
    }
    float* dst = out + (int64_t)o * C + c;
    if constexpr (V == 4) *reinterpret_cast<float4*>(dst) = make_float4(m[0], m[1], m[2], m[3]);
    else dst[0] = m[0];
}

extern "C" int al3d_sp_maxpool_f32(const float* feats, const int* nbr, int64_t ld, int K, int C, int n_out, int zero_floor,
                                   float* out, void* stream)
{
    AL3D_REQUIRE(K >= 1 && C >= 1 && n_out >= 0 && ld >= n_out, "al3d_sp_maxpool_f32: bad sizes");
    if (n_out == 0) return AL3D_OK;
    AL3D_REQUIRE(feats && nbr && out, "al3d_sp_maxpool_f32: null pointer");
    hipStream_t s = (hipStream_t)stream;
    if (C % 4 == 0 && (((uintptr_t)feats | (uintptr_t)out) & 15) == 0) {
        hipLaunchKernelGGL(sm_maxpool_kernel<4>, dim3(sm_blocks((int64_t)n_out * (C / 4), 256)), dim3(256), 0, s, feats, nbr, ld,
                           K, C, n_out, zero_floor, out);
    } else {
        hipLaunchKernelGGL(sm_maxpool_kernel<1>, dim3(sm_blocks((int64_t)n_out * C, 256)), dim3(256), 0, s, feats, nbr, ld, K, C,
                           n_out, zero_floor, out);
    }
    AL3D_CHECK_LAUNCH("sm_maxpool_kernel");
    return AL3D_OK;
}

// ------------------------------------------------------------------ inverse table
// nbr_inv[k][i] = o where nbr_fwd[k][o] == i.  For a given tap an input cell belongs to at most one output cell
// (o = (i + p - d_k) / s), so every entry has one writer; the table is pre-filled with -1.
template <bool TILES>
__global__ void sm_inverse_table_kernel(const int* __restrict__ nbr_fwd, int64_t ld_fwd, int K, int n_out, int n_in,
                                        int* __restrict__ nbr_inv, int64_t ld_inv, unsigned* __restrict__ tmask)
{
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (int64_t)K * n_out) return;
    const int k = (int)(e / n_out), o = (int)(e % n_out);
    const int i = nbr_fwd[(int64_t)k * ld_fwd + o];
    if (i < 0 || i >= n_in) return;
    nbr_inv[(int64_t)k * ld_inv + i] = o;
    if constexpr (TILES) atomicOr(&tmask[i >> 5], 1u << k);
}

static int sm_inverse_table(const int* nbr_fwd, int64_t ld_fwd, int K, int n_out, int n_in, int* nbr_inv, int64_t ld_inv,
                            unsigned* tmask, void* stream)
{
    AL3D_REQUIRE(K >= 1 && K <= 27 && n_out >= 0 && n_in >= 0 && ld_fwd >= n_out && ld_inv >= n_in && ld_inv >= 1,
                 "al3d_sp_inverse_table: bad sizes");
    AL3D_REQUIRE(nbr_inv && (n_out == 0 || nbr_fwd), "al3d_sp_inverse_table: null pointer");
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(nbr_inv, 0xff, (size_t)K * ld_inv * 4, s) != hipSuccess ||
        (tmask && hipMemsetAsync(tmask, 0, (size_t)(ld_inv / 32) * 4, s) != hipSuccess))
        return al3d_fail(AL3D_ELAUNCH, "al3d_sp_inverse_table: memset failed");
    if (n_out == 0 || n_in == 0) return AL3D_OK;
    const dim3 grid(sm_blocks((int64_t)K * n_out, 256));
    if (tmask)
        hipLaunchKernelGGL(sm_inverse_table_kernel<true>, grid, dim3(256), 0, s, nbr_fwd, ld_fwd, K, n_out, n_in, nbr_inv, ld_inv,
                           tmask);
    else
        hipLaunchKernelGGL(sm_inverse_table_kernel<false>, grid, dim3(256), 0, s, nbr_fwd, ld_fwd, K, n_out, n_in, nbr_inv,
                           ld_inv, tmask);
    AL3D_CHECK_LAUNCH("sm_inverse_table_kernel");
    return AL3D_OK;
}

extern "C" int al3d_sp_inverse_table(const int* nbr_fwd, int64_t ld_fwd, int K, int n_out, int n_in, int* nbr_inv,
                                     void* stream)
{
    return sm_inverse_table(nbr_fwd, ld_fwd, K, n_out, n_in, nbr_inv, n_in > 0 ? n_in : 1, nullptr, stream);
}

extern "C" int al3d_sp_inverse_table_tiles(const int* nbr_fwd, int64_t ld_fwd, int K, int n_out, int n_in, int* nbr_inv,
                                           int pitch, unsigned* tile_mask, void* stream)
{
    AL3D_REQUIRE(n_in >= 0 && pitch == al3d_sp_table_pitch(n_in) && tile_mask,
                 "al3d_sp_inverse_table_tiles: pitch must be al3d_sp_table_pitch(n_in), tile_mask non-null");
    return sm_inverse_table(nbr_fwd, ld_fwd, K, n_out, n_in, nbr_inv, pitch, tile_mask, stream);
}

// ------------------------------------------------------------------ transposed conv: output sites
// al3d_sp_down_sites (csrc/spconv.hip) with the transposed rule in the marking pass: every input marks the cells i*s - p + d
// it feeds (one byte per cell, plain idempotent stores); the numbering passes are that entry point's own (sp_sites.h).
__global__ void sm_up_mark_kernel(const int* __restrict__ coords_in, int n_in, SmGeom q, SmDims go,
                                  unsigned char* __restrict__ flags)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_in) return;
    const int4 c = *reinterpret_cast<const int4*>(coords_in + 4 * (int64_t)i);
    const int z0 = c.y * q.sd - q.pd, y0 = c.z * q.sh - q.ph, x0 = c.w * q.sw - q.pw;
    for (int kz = 0; kz < q.kd; ++kz) {
        const int z = z0 + kz;
        if (z < 0 || z >= go.D) continue;
        for (int ky = 0; ky < q.kh; ++ky) {
            const int y = y0 + ky;
            if (y < 0 || y >= go.H) continue;
            for (int kx = 0; kx < q.kw; ++kx) {
                const int x = x0 + kx;
                if (x < 0 || x >= go.W) continue;
                flags[sm_cell(go, c.x, z, y, x)] = 1;
            }
        }
    }
}

extern "C" int64_t al3d_sp_up_sites_workspace_bytes(int B, int OD, int OH, int OW)
{
    return al3d_sp_down_sites_workspace_bytes(B, OD, OH, OW);
}

extern "C" int al3d_sp_up_sites(const int* coords_in, int n_in, const int* ksize, const int* stride, const int* pad, int B,
                                int OD, int OH, int OW, int* grid_out, int* coords_out, int* counter, int cap, void* workspace,
                                void* stream)
{
    AL3D_REQUIRE(ksize && stride && pad && grid_out && coords_out && counter && workspace, "al3d_sp_up_sites: null pointer");
    AL3D_REQUIRE(n_in >= 0 && B >= 1 && OD >= 1 && OH >= 1 && OW >= 1, "al3d_sp_up_sites: bad sizes");
    const int64_t cells = (int64_t)B * OD * OH * OW;
    AL3D_REQUIRE(cells < (1LL << 31), "al3d_sp_up_sites: B*OD*OH*OW must be below 2^31");
    for (int d = 0; d < 3; ++d)
        AL3D_REQUIRE(ksize[d] >= 1 && stride[d] >= 1 && pad[d] >= 0, "al3d_sp_up_sites: bad geometry");
    AL3D_REQUIRE(((uintptr_t)coords_out & 15) == 0 && ((uintptr_t)workspace & 15) == 0 && ((uintptr_t)coords_in & 15) == 0,
                 "al3d_sp_up_sites: coords_in / coords_out / workspace must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    if (n_in == 0) {
        if (hipMemsetAsync(counter, 0, 4, s) != hipSuccess) return al3d_fail(AL3D_ELAUNCH, "al3d_sp_up_sites: memset failed");
        return AL3D_OK;
    }
    AL3D_REQUIRE(coords_in, "al3d_sp_up_sites: null coords");
    const int64_t words = (cells + 31) / 32;
    unsigned char* flags = (unsigned char*)workspace;
    if (hipMemsetAsync(flags, 0, (size_t)words * 32, s) != hipSuccess)
        return al3d_fail(AL3D_ELAUNCH, "al3d_sp_up_sites: memset failed");
    SmGeom q = {ksize[0], ksize[1], ksize[2], stride[0], stride[1], stride[2], pad[0], pad[1], pad[2]};
    SmDims go = {B, OD, OH, OW};
    hipLaunchKernelGGL(sm_up_mark_kernel, dim3(sm_blocks(n_in, 256)), dim3(256), 0, s, coords_in, n_in, q, go, flags);
    const int rc = al3d_sp_number_marked_raster(workspace, B, OD, OH, OW, grid_out, coords_out, counter, cap, s);
    if (rc) return rc;
    AL3D_CHECK_LAUNCH("al3d_sp_up_sites");
    return AL3D_OK;
}

// ------------------------------------------------------------------ transposed conv: table
// nbr[k][o] = the input row at (o + p - d_k) / s where that division is exact in all three dimensions and the cell is inside
// the input grid, else -1.  One thread per (tap, output row), tap-major: coalesced table stores.  Exact grids of pitch * K
// threads for the tiled form (pitch is a multiple of 256), whose waves cover two 32-row tiles.
template <bool TILES>
__global__ void sm_up_table_kernel(const int* __restrict__ coords_out, int n_out, int64_t ld, SmGeom q, SmDims gi,
                                   const int* __restrict__ grid_in, int* __restrict__ nbr, unsigned* __restrict__ tmask)
{
    const int K = q.kd * q.kh * q.kw;
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (int64_t)K * ld) return;
    const int k = (int)(e / ld), o = (int)(e % ld);
    int v = -1;
    if (o < n_out) {
        const int4 c = *reinterpret_cast<const int4*>(coords_out + 4 * (int64_t)o);
        const int kx = k % q.kw, ky = (k / q.kw) % q.kh, kz = k / (q.kw * q.kh);
        const int nz = c.y + q.pd - kz, ny = c.z + q.ph - ky, nx = c.w + q.pw - kx;
        if (nz >= 0 && ny >= 0 && nx >= 0 && nz % q.sd == 0 && ny % q.sh == 0 && nx % q.sw == 0) {
            const int z = nz / q.sd, y = ny / q.sh, x = nx / q.sw;
            if (z < gi.D && y < gi.H && x < gi.W) v = grid_in[sm_cell(gi, c.x, z, y, x)];
        }
    }
    nbr[(int64_t)k * ld + o] = v;
    if constexpr (TILES) {
        const int lane = threadIdx.x & 63;
        const unsigned long long bal = __ballot(v >= 0);
        if (lane == 0 && (bal & 0xffffffffull)) atomicOr(&tmask[o >> 5], 1u << k);
        if (lane == 32 && (bal >> 32)) atomicOr(&tmask[o >> 5], 1u << k);
    }
}

static int sm_up_table(const int* coords_out, int n_out, const int* ksize, const int* stride, const int* pad, int B, int ID,
                       int IH, int IW, const int* grid_in, int* nbr, int64_t ld, unsigned* tmask, void* stream)
{
    AL3D_REQUIRE(ksize && stride && pad && nbr && n_out >= 0 && (n_out == 0 || (coords_out && grid_in)),
                 "al3d_sp_up_table: null pointer");
    for (int d = 0; d < 3; ++d)
        AL3D_REQUIRE(ksize[d] >= 1 && stride[d] >= 1 && pad[d] >= 0, "al3d_sp_up_table: bad geometry");
    const int K = ksize[0] * ksize[1] * ksize[2];
    AL3D_REQUIRE(K <= 27, "al3d_sp_up_table: at most 27 taps");
    AL3D_REQUIRE(((uintptr_t)coords_out & 15) == 0, "al3d_sp_up_table: coords_out must be 16-byte aligned");
    AL3D_REQUIRE((int64_t)B * ID * IH * IW < (1LL << 31), "al3d_sp_up_table: B*ID*IH*IW must be below 2^31");
    hipStream_t s = (hipStream_t)stream;
    SmGeom q = {ksize[0], ksize[1], ksize[2], stride[0], stride[1], stride[2], pad[0], pad[1], pad[2]};
    SmDims gi = {B, ID, IH, IW};
    if (tmask) {
        if (hipMemsetAsync(tmask, 0, (size_t)(ld / 32) * 4, s) != hipSuccess)
            return al3d_fail(AL3D_ELAUNCH, "al3d_sp_up_table_tiles: memset failed");
        hipLaunchKernelGGL(sm_up_table_kernel<true>, dim3((unsigned)(K * ld / 256)), dim3(256), 0, s, coords_out, n_out, ld, q,
                           gi, grid_in, nbr, tmask);
    } else {
        if (n_out == 0) return AL3D_OK;
        hipLaunchKernelGGL(sm_up_table_kernel<false>, dim3(sm_blocks((int64_t)K * ld, 256)), dim3(256), 0, s, coords_out, n_out,
                           ld, q, gi, grid_in, nbr, tmask);
    }
    AL3D_CHECK_LAUNCH("sm_up_table_kernel");
    return AL3D_OK;
}

extern "C" int al3d_sp_up_table(const int* coords_out, int n_out, const int* ksize, const int* stride, const int* pad, int B,
                                int ID, int IH, int IW, const int* grid_in, int* nbr, void* stream)
{
    return sm_up_table(coords_out, n_out, ksize, stride, pad, B, ID, IH, IW, grid_in, nbr, n_out, nullptr, stream);
}

extern "C" int al3d_sp_up_table_tiles(const int* coords_out, int n_out, const int* ksize, const int* stride, const int* pad,
                                      int B, int ID, int IH, int IW, const int* grid_in, int* nbr, int pitch,
                                      unsigned* tile_mask, void* stream)
{
    AL3D_REQUIRE(n_out >= 0 && pitch == al3d_sp_table_pitch(n_out) && tile_mask,
                 "al3d_sp_up_table_tiles: pitch must be al3d_sp_table_pitch(n_out), tile_mask non-null");
    return sm_up_table(coords_out, n_out, ksize, stride, pad, B, ID, IH, IW, grid_in, nbr, pitch, tile_mask, stream);
}

// ------------------------------------------------------------------ VALU convolution, any channel pair
// out[o][co] = (sum over k, then ci, in that order, of in[nbr[k][o]][ci] * w[k][ci][co], one f32 FMA chain) * scale + shift
// (+ residual) (ReLU; NaN stays NaN).  One thread per output element: the lanes of a row read consecutive weights, the
// gathered value is the same word for all of them.  For the pairs al3d_sp_conv_f32 has no instantiation of.
__global__ void sm_conv_any_kernel(const float* __restrict__ fin, const int* __restrict__ nbr, int K, const float* __restrict__ wgt,
                                   int cin, int cout, const float* __restrict__ scale, const float* __restrict__ shift,
                                   const float* __restrict__ residual, int relu, float* __restrict__ fout, int n_out)
{
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (int64_t)n_out * cout) return;
    const int o = (int)(e / cout), co = (int)(e % cout);
    float acc = 0.f;
    for (int k = 0; k < K; ++k) {
        const int i = nbr[(int64_t)k * n_out + o];
        if (i < 0) continue;
        const float* x = fin + (int64_t)i * cin;
        const float* w = wgt + (int64_t)k * cin * cout + co;
        for (int ci = 0; ci < cin; ++ci) acc = fmaf(x[ci], w[(int64_t)ci * cout], acc);
    }
    float v = acc;
    if (scale) v *= scale[co];
    if (shift) v += shift[co];
    if (residual) v += residual[e];
    if (relu) v = v <= 0.f ? 0.f : v;
    fout[e] = v;
}

extern "C" int al3d_sp_conv_any_f32(const float* fin, const int* nbr, int K, const float* wgt, int cin, int cout,
                                    const float* scale, const float* shift, const float* residual, int relu, float* fout,
                                    int n_out, void* stream)
{
    AL3D_REQUIRE(K >= 1 && n_out >= 0 && cin >= 1 && cout >= 1, "al3d_sp_conv_any_f32: bad sizes");
    if (n_out == 0) return AL3D_OK;
    AL3D_REQUIRE(fin && nbr && wgt && fout, "al3d_sp_conv_any_f32: null pointer");
    hipLaunchKernelGGL(sm_conv_any_kernel, dim3(sm_blocks((int64_t)n_out * cout, 256)), dim3(256), 0, (hipStream_t)stream, fin,
                       nbr, K, wgt, cin, cout, scale, shift, residual, relu, fout, n_out);
    AL3D_CHECK_LAUNCH("sm_conv_any_kernel");
    return AL3D_OK;
}
