// Dense 2-D convolution in bf16x6 arithmetic: fp32-faithful on the bf16 matrix cores (gfx950).  The arithmetic -- the
// exact three-way split, the six products and their order -- is al3d_bf16x6.h's.
//
// Same role, layouts and tiling as conv2d_mfma.hip (NHWC f32 activations in HBM; 128 px x 128
// ch tile; 4 waves 2x2; double-buffered LDS); activations are split while they are staged
// (registers -> LDS), weights are pre-split once into [3][Cout][taps][Cin] bf16.  The pixel-tile side (parameter block, tile
// decode, input pixel, epilogues, entry-point checks) is conv2d_tile.h's.
#include "al3d_common.h"
#include "al3d_bf16x6.h"
#include "conv2d_tile.h"

#define C6_BM 128
#define C6_BN 128
#define C6_BK 16
#define C6_TH 8
#define C6_TW 16

struct Conv6Params : ConvGeom {
    const __bf16* wgt;      // [3][Cout][taps][Cin] bf16 planes (hi, mid, lo)
    int64_t plane;          // elements per weight plane = Cout * taps * Cin
};

// MODE 0: convolution, a tile = 8 x 16 output pixels.  MODE 1: 2x2 stride-2 deconvolution, a tile = 8 x 16 INPUT pixels
// and blockIdx.z = the tap, i.e. which of the four output pixels of each input pixel.  The loop is b6_tile_pipeline.
template <int MODE>
__global__ __launch_bounds__(256, 2) void conv2d_bf16x6_kernel(Conv6Params p)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm = wave & 1, wn = wave >> 1;
    int tx_, ty_, b;
    conv_tile_decode(blockIdx.x, p.tiles_x, p.tiles_y, tx_, ty_, b);
    const int n0 = blockIdx.y * C6_BN;
    const int taps = MODE == 0 ? p.ksize * p.ksize : 1;
    const int tap0 = MODE == 0 ? 0 : blockIdx.z;
    const int wtaps = MODE == 0 ? taps : 4;
    const int kchunks = p.Cin / C6_BK;

    // step = tap * kchunks + chunk (the deconvolution has one tap per launch); A row m of the tile = pixel (m / 16, m % 16)
    auto tap_of = [&](int step) { return MODE == 0 ? step / kchunks : 0; };
    auto load_a = [&](int step, int row, int q, float4 (&ra)[2]) {
        const int tap = tap_of(step), c0 = (step - tap * kchunks) * C6_BK;
        const int ky = MODE == 0 ? tap / p.ksize : 0, kx = MODE == 0 ? tap % p.ksize : 0;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int m = row + 64 * i;
            const int py = ty_ * C6_TH + m / C6_TW, px = tx_ * C6_TW + m % C6_TW;
            int iy, ix;
            const bool ok = conv_tap_pixel<MODE>(p, py, px, ky, kx, iy, ix);
            ra[i] = conv_load4(p, ok, b, iy, ix, c0 + 4 * q);
        }
    };
    auto load_b = [&](int step, int row, int q, uint4 (&rb)[3]) {
        const int tap = tap_of(step), c0 = (step - tap * kchunks) * C6_BK;
        const int n = n0 + row;
#pragma unroll
        for (int pl = 0; pl < 3; ++pl)
            rb[pl] = n < p.Cout ? *reinterpret_cast<const uint4*>(
                                      p.wgt + pl * p.plane + ((int64_t)n * wtaps + tap0 + tap) * p.Cin + c0 + 8 * q)
                                : make_uint4(0u, 0u, 0u, 0u);
    };
    f32x16 acc[2][2];
    b6_tile_pipeline(taps * kchunks, load_a, load_b, acc);

    conv_store_patch<MODE, C6_TH, C6_TW, 2, 2, true, false>(p, acc, b, ty_, tx_, wm, n0 + wn * 64, tap0, lane);
}

// ------------------------------------------------------------------ 3x3 / stride 1 / pad 1
// The generic kernel above re-stages (and re-splits) every input pixel once per filter tap, and
// its LDS write traffic (activations + weights, 24 KB per step) is what bounds it.  For the
// twelve 3x3 stride-1 layers of the neck the input halo of the output tile is staged ONCE per
// 16-channel chunk -- 6x34 pixels for a 4x32 output tile -- and the nine taps read their A
// fragments from it at shifted rows; only the weight tile changes per tap.  LDS writes per
// step drop from 24 KB to ~14 KB and the split arithmetic by 6x.
// Output tile = 4 rows x 32 columns: lane r of an M-tile is column r, so the 32 lanes of a
// fragment read 32 consecutive halo rows (conflict-free ds_read_b128 at a 48-byte pitch).
#define H3_TH 4
#define H3_TW 32
#define H3_HH (H3_TH + 2)
#define H3_HW (H3_TW + 2)
#define H3_HP (H3_HH * H3_HW)          // 204 halo pixels

// Software pipeline: a tap that starts with its twelve ds_read_b128 right after the barrier has
// nothing to cover their latency (measured: +4 % when removed).  The fragments of tap t+1 are read
// into a second register set while the 24 MFMAs of tap t run, so a step opens with MFMAs whose
// operands are already in registers:
//   * weights live in THREE LDS buffers (tap t, t+1 readable; t+2 being written) -- 32-byte rows
//     with the 16-byte halves XOR-swizzled by bit 3 of the row (conflict-free ds_read_b128 /
//     ds_write_b128 without the 16-byte pad), so three buffers cost what two padded ones did;
//   * still one barrier per tap: it publishes B(t+2) and retires B(t) (whose fragments were
//     read during tap t-1);
//   * the next chunk's halo is stored during tap 8 (its fragments were read during tap 7) and
//     published by tap 8's barrier; only tap 0 of a chunk reads its fragments unprefetched.
#define H3_BROW 32                     // bytes per weight row in LDS (16 bf16, swizzled halves)
__global__ __launch_bounds__(256, 2) void conv3x3_bf16x6_halo_kernel(Conv6Params p)
{
    __shared__ __attribute__((aligned(16))) unsigned char Ah[3][H3_HP * B6_PITCH];          // 29.4 KB
    __shared__ __attribute__((aligned(16))) unsigned char Bs[3][3][C6_BN * H3_BROW];     // 36.9 KB
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int wm = wave & 1, wn = wave >> 1;
    const int fr = lane & 31, fh = lane >> 5;
    int tx_, ty_, b;
    conv_tile_decode(blockIdx.x, p.tiles_x, p.tiles_y, tx_, ty_, b);
    const int n0 = blockIdx.y * C6_BN;
    const int y0 = ty_ * H3_TH - 1, x0 = tx_ * H3_TW - 1;       // image coords of halo (0,0)
    const int nchunks = p.Cin / C6_BK;
    const int bq = tid & 1, br = tid >> 1;

    float4 rh[4];
    uint4 rb[3];
    auto load_halo = [&](int chunk) {
        const int c0 = chunk * C6_BK;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int piece = tid + 256 * i;
            const int hp = piece >> 2, q = piece & 3;
            int iy, ix;
            const bool ok = conv_halo_pixel<H3_HW>(p, y0, x0, hp, hp < H3_HP, iy, ix);
            rh[i] = conv_load4(p, ok, b, iy, ix, c0 + 4 * q);
        }
    };
    auto store_halo = [&]() {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int piece = tid + 256 * i;
            const int hp = piece >> 2, q = piece & 3;
            if (hp >= H3_HP) continue;
            b6_stage4(Ah, hp * B6_PITCH + 8 * q, rh[i]);
        }
    };
    const int nb = n0 + br;
    const bool nb_ok = nb < p.Cout;
    const __bf16* wrow = p.wgt + (int64_t)nb * 9 * p.Cin + 8 * bq;     // this thread's weight row
    auto load_b = [&](int chunk, int tap) {
#pragma unroll
        for (int pl = 0; pl < 3; ++pl)
            rb[pl] = nb_ok ? *reinterpret_cast<const uint4*>(wrow + pl * p.plane + tap * p.Cin + chunk * C6_BK)
                           : make_uint4(0u, 0u, 0u, 0u);
    };
    const int bw_off = br * H3_BROW + 16 * (bq ^ ((br >> 3) & 1));
    auto store_b = [&](int buf) {
#pragma unroll
        for (int pl = 0; pl < 3; ++pl)
            *reinterpret_cast<uint4*>(&Bs[buf][pl][bw_off]) = rb[pl];
    };

    f32x16 acc[2][2];
    conv_acc_clear(acc);

    const int total = 9 * nchunks;                    // steps; step s = chunk * 9 + tap, B(s) lives in buffer tap % 3
    load_halo(0);
    load_b(0, 0);
    store_halo();
    store_b(0);
    load_b(0, 1);
    store_b(1);
    __syncthreads();
    const int a_off = ((2 * wm) * H3_HW + fr) * B6_PITCH + 16 * fh;
    const int b_off = (wn * 64 + fr) * H3_BROW + 16 * (fh ^ ((fr >> 3) & 1));   // +32 rows keeps bit 3
    // [set][tile]; read plane-major with A and B interleaved, not fragment by fragment: that issue order is one VGPR
    // cheaper here (and the weight rows are 32-byte swizzled rows, not b6_frag's)
    B6Frag fa[2][2], fb[2][2];
    for (int chunk = 0; chunk < nchunks; ++chunk) {
        const bool more = chunk + 1 < nchunks;
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {           // compile-time taps: immediate LDS offsets, static sets
            const int cs = tap & 1, ns = cs ^ 1;
            // ---- weights two steps ahead (registers now, LDS at the end of the step)
            const bool has2 = chunk * 9 + tap + 2 < total;
            if (tap < 7) load_b(chunk, tap + 2);
            else if (more) load_b(chunk + 1, tap - 7);
            if (tap == 0 && more) load_halo(chunk + 1);             // lands during the 9 taps
            if (tap == 0) {                                         // first tap of a chunk: fragments not prefetched
#pragma unroll
                for (int pl = 0; pl < 3; ++pl)
#pragma unroll
                    for (int t = 0; t < 2; ++t) {
                        fa[0][t].p[pl] = *reinterpret_cast<const bf16x8*>(&Ah[pl][a_off + (t * H3_HW) * B6_PITCH]);
                        fb[0][t].p[pl] = *reinterpret_cast<const bf16x8*>(&Bs[0][pl][b_off + t * 32 * H3_BROW]);
                    }
            }
            if (tap < 8) {                                          // fragments of the next tap
                const int ky = (tap + 1) / 3, kx = (tap + 1) % 3;
#pragma unroll
                for (int pl = 0; pl < 3; ++pl)
#pragma unroll
                    for (int t = 0; t < 2; ++t) {
                        fa[ns][t].p[pl] = *reinterpret_cast<const bf16x8*>(
                            &Ah[pl][a_off + ((t + ky) * H3_HW + kx) * B6_PITCH]);
                        fb[ns][t].p[pl] = *reinterpret_cast<const bf16x8*>(
                            &Bs[(tap + 1) % 3][pl][b_off + t * 32 * H3_BROW]);
                    }
            }
            if (tap == 8 && more) store_halo();                     // halo(chunk) was last read during tap 7
            // product-major over the four tiles: four independent accumulators between two MFMAs into the same one
#pragma unroll
            for (int t = 0; t < 6; ++t)
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j) b6_product(t, fa[cs][i], fb[cs][j], acc[i][j]);
            if (has2) store_b((tap + 2) % 3);
            __syncthreads();
        }
    }

    conv_store_rows<H3_TH, H3_TW, 2, 2, true>(p, acc, b, ty_, tx_, 2 * wm, n0 + wn * 64, lane);
}

// one-off weight split: f32 [count] -> bf16 [3][count]
__global__ void split_weights_kernel(const float* __restrict__ w, int64_t count, __bf16* __restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    __bf16 a, b, c;
    b6_split(w[i], a, b, c);
    out[i] = a; out[count + i] = b; out[2 * count + i] = c;
}

extern "C" int al3d_split_bf16x3(const float* w, int64_t count, void* out_bf16x3, void* stream)
{
    AL3D_REQUIRE(w && out_bf16x3 && count >= 0, "al3d_split_bf16x3: bad arguments");
    if (count == 0) return AL3D_OK;
    hipLaunchKernelGGL(split_weights_kernel, dim3((unsigned)al3d_cdiv(count, 256)), dim3(256), 0,
                       (hipStream_t)stream, w, count, (__bf16*)out_bf16x3);
    AL3D_CHECK_LAUNCH("split_weights_kernel");
    return AL3D_OK;
}

// inverse of the split: f32 = (x1 + x2) + x3, exact
__global__ void merge_planes_kernel(const __bf16* __restrict__ pl, int64_t count, float* __restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    out[i] = ((float)pl[i] + (float)pl[count + i]) + (float)pl[2 * count + i];
}

extern "C" int al3d_merge_bf16x3(const void* planes_bf16x3, int64_t count, float* out, void* stream)
{
    AL3D_REQUIRE(count >= 0, "al3d_merge_bf16x3: bad count");
    if (count == 0) return AL3D_OK;
    AL3D_REQUIRE(planes_bf16x3 && out, "al3d_merge_bf16x3: null pointer");
    hipLaunchKernelGGL(merge_planes_kernel, dim3((unsigned)al3d_cdiv(count, 256)), dim3(256), 0,
                       (hipStream_t)stream, (const __bf16*)planes_bf16x3, count, out);
    AL3D_CHECK_LAUNCH("merge_planes_kernel");
    return AL3D_OK;
}

extern "C" int al3d_conv2d_nhwc_bf16x6(const float* in, const void* wgt_bf16x3, const float* scale,
                                       const float* shift, float* out, int B, int H, int W, int Cin,
                                       int Cout, int ksize, int stride, int pad, int ldc, int coff,
                                       int relu, void* stream)
{
    const bool halo = ksize == 3 && stride == 1 && pad == 1;     // halo-staged fast path
    Conv6Params p;
    p.wgt = (const __bf16*)wgt_bf16x3;
    p.plane = (int64_t)Cout * ksize * ksize * Cin;
    int rc = conv_geom_build(p, "al3d_conv2d_nhwc_bf16x6", false, halo ? H3_TH : C6_TH, halo ? H3_TW : C6_TW, C6_BK, false, in,
                             wgt_bf16x3, scale, shift, out, B, H, W, Cin, Cout, ksize, stride, pad, ldc, coff, relu);
    if (rc) return rc;
    dim3 grid((unsigned)(p.tiles_x * p.tiles_y * B), (unsigned)al3d_cdiv(Cout, C6_BN), 1);
    if (halo) {
        hipLaunchKernelGGL(conv3x3_bf16x6_halo_kernel, grid, dim3(256), 0, (hipStream_t)stream, p);
        AL3D_CHECK_LAUNCH("conv3x3_bf16x6_halo_kernel");
        return AL3D_OK;
    }
    hipLaunchKernelGGL(conv2d_bf16x6_kernel<0>, grid, dim3(256), 0, (hipStream_t)stream, p);
    AL3D_CHECK_LAUNCH("conv2d_bf16x6_kernel<conv>");
    return AL3D_OK;
}

extern "C" int al3d_deconv2x2_nhwc_bf16x6(const float* in, const void* wgt_bf16x3, const float* scale,
                                          const float* shift, float* out, int B, int H, int W, int Cin,
                                          int Cout, int ldc, int coff, int relu, void* stream)
{
    Conv6Params p;
    p.wgt = (const __bf16*)wgt_bf16x3;
    p.plane = (int64_t)Cout * 4 * Cin;
    int rc = conv_geom_build(p, "al3d_deconv2x2_nhwc_bf16x6", true, C6_TH, C6_TW, C6_BK, false, in, wgt_bf16x3, scale, shift, out,
                             B, H, W, Cin, Cout, 2, 2, 0, ldc, coff, relu);
    if (rc) return rc;
    dim3 grid((unsigned)(p.tiles_x * p.tiles_y * B), (unsigned)al3d_cdiv(Cout, C6_BN), 4);
    hipLaunchKernelGGL(conv2d_bf16x6_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, p);
    AL3D_CHECK_LAUNCH("conv2d_bf16x6_kernel<deconv>");
    return AL3D_OK;
}
