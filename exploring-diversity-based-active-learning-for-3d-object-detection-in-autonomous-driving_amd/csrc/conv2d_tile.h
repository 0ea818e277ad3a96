// The pixel-tile side of the dense 2-D convolution kernels, once for all three arithmetics (conv2d_mfma.hip,
// conv2d_bf16x6.hip, conv2d_f16x3.hip, conv2d_wino.hip, conv2d_res.hip): the geometry block of their parameter structs,
// the host-side builder and argument check, and the device pieces that turn a workgroup into a pixel tile, a tile pixel
// and a filter tap into an input address, and an accumulator fragment into NHWC stores inside a channel window.
//
// What stays with its kernel: staging, pipelines and product loops; every epilogue that goes through LDS (the transposing
// stores of conv3x3_f16x3_frag_kernel and conv2d_f16x3_dma2_kernel, the Winograd output exchange); the residual kernel's
// epilogue (it adds the residual between the affine and the ReLU); conv3x3_f16x3_frag16_kernel's (16 x 16 fragments).
//
// Everything here is __forceinline__ and takes its operands by value or through the kernel's own parameter block, so a
// kernel's code is what its private copy gave (profiles/conv2d_tile_parent_vs_tree.md).
#pragma once
#include "al3d_common.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));      // the same typedef as the arithmetic headers' (all may be included)

// ------------------------------------------------------------------ parameter block
// The fields every dense kernel reads.  ConvParams, Conv6Params, ConvF3Params, WinoParams and ConvResParams derive from
// it and add their weight pointer and what is their own.
struct ConvGeom {
    const float* in;        // [B, H, W, Cin] f32
    const float* scale;     // [Cout], or null (= 1) where the arithmetic allows it
    const float* shift;     // [Cout] or null (= 0)
    float* out;             // [B, OH, OW, ldc], written at channel offset coff
    int B, H, W, Cin, Cout, OH, OW, ldc, coff;
    int ksize, stride, pad, relu;
    int tiles_x, tiles_y;   // th x tw pixel tiles per image, over the GEMM-M pixel grid (deconvolution: the input map)
};

// ------------------------------------------------------------------ host: one builder, one check
// Fields, output size and tile counts.  deconv: the 2x2 / stride-2 transposed convolution (ksize, stride, pad = 2, 2, 0;
// pixel tiles over the input map).  The caller has checked stride >= 1.
static inline void conv_geom_set(ConvGeom& g, bool deconv, int th, int tw, const float* in, const float* scale,
                                 const float* shift, float* out, int B, int H, int W, int Cin, int Cout, int ksize, int stride,
                                 int pad, int ldc, int coff, int relu)
{
    g.in = in; g.scale = scale; g.shift = shift; g.out = out;
    g.B = B; g.H = H; g.W = W; g.Cin = Cin; g.Cout = Cout;
    g.ksize = ksize; g.stride = stride; g.pad = pad; g.ldc = ldc; g.coff = coff; g.relu = relu;
    g.OH = deconv ? 2 * H : (H + 2 * pad - ksize) / stride + 1;
    g.OW = deconv ? 2 * W : (W + 2 * pad - ksize) / stride + 1;
    g.tiles_x = (int)al3d_cdiv(deconv ? W : g.OW, tw);
    g.tiles_y = (int)al3d_cdiv(deconv ? H : g.OH, th);
}

// The five requirements of every entry point; bk = input channels per step, need_scale: the f16x3 kernels (their scale
// carries the weight exponent)
static inline int conv_geom_check(const ConvGeom& g, const void* wgt, const char* name, int bk, bool need_scale)
{
    if (need_scale)
        AL3D_REQUIRE(g.in && wgt && g.out && g.scale, "%s: null pointer (scale carries the weight exponent and is required)", name);
    else
        AL3D_REQUIRE(g.in && wgt && g.out, "%s: null pointer", name);
    AL3D_REQUIRE(g.B >= 1 && g.H >= 1 && g.W >= 1 && g.Cin >= 1 && g.Cout >= 1, "%s: bad shape", name);
    AL3D_REQUIRE(g.Cin % bk == 0, "%s: Cin=%d must be a multiple of %d", name, g.Cin, bk);
    AL3D_REQUIRE(g.coff >= 0 && g.coff + g.Cout <= g.ldc, "%s: channel window [%d,%d) exceeds ldc=%d",
                 name, g.coff, g.coff + g.Cout, g.ldc);
    AL3D_REQUIRE(((uintptr_t)g.in & 15) == 0 && ((uintptr_t)wgt & 15) == 0,
                 "%s: in/wgt must be 16-byte aligned", name);
    return AL3D_OK;
}

// Checks the arguments of entry point `name` and fills g for th x tw pixel tiles
static inline int conv_geom_build(ConvGeom& g, const char* name, bool deconv, int th, int tw, int bk, bool need_scale,
                                  const float* in, const void* wgt, const float* scale, const float* shift, float* out, int B,
                                  int H, int W, int Cin, int Cout, int ksize, int stride, int pad, int ldc, int coff, int relu)
{
    AL3D_REQUIRE(ksize >= 1 && ksize <= 7 && stride >= 1 && pad >= 0, "%s: bad geometry", name);
    conv_geom_set(g, deconv, th, tw, in, scale, shift, out, B, H, W, Cin, Cout, ksize, stride, pad, ldc, coff, relu);
    AL3D_REQUIRE(deconv || (g.OH >= 1 && g.OW >= 1), "%s: empty output", name);
    return conv_geom_check(g, wgt, name, bk, need_scale);
}

// ------------------------------------------------------------------ device: tile, input pixel, accumulators
// pixel-tile index -> tile column, tile row, image (tiles run x-fastest, then y, then the batch)
__device__ __forceinline__ void conv_tile_decode(int tile, int tiles_x, int tiles_y, int& tx, int& ty, int& b)
{
    tx = tile % tiles_x; tile /= tiles_x;
    ty = tile % tiles_y; tile /= tiles_y;
    b = tile;
}

// C/D fragment of the 32 x 32 MFMAs: register r of lane half fh holds this row (the column is lane & 31)
__device__ __forceinline__ int mfma32_crow(int r, int fh) { return (r & 3) + 8 * (r >> 2) + 4 * fh; }

template <int NI, int NJ> __device__ __forceinline__ void conv_acc_clear(f32x16 (&acc)[NI][NJ])
{
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
}

// Pixel (py, px) of the GEMM-M grid at filter tap (ky, kx): MODE 0 reads input pixel (py * stride - pad + ky, ...), MODE 1
// (deconvolution) the pixel itself.  False past the ragged edge of the tile grid and outside the image (zero padding).
template <int MODE>
__device__ __forceinline__ bool conv_tap_pixel(const ConvGeom& g, int py, int px, int ky, int kx, int& iy, int& ix)
{
    const int MH = MODE == 0 ? g.OH : g.H, MW = MODE == 0 ? g.OW : g.W;
    if (MODE == 0) { iy = py * g.stride - g.pad + ky; ix = px * g.stride - g.pad + kx; }
    else { iy = py; ix = px; }
    return py < MH && px < MW && iy >= 0 && iy < g.H && ix >= 0 && ix < g.W;
}

// Halo form: halo pixel hp of a halo HW pixels wide whose corner is image pixel (y0, x0); inside = the bound on the piece index
template <int HW>
__device__ __forceinline__ bool conv_halo_pixel(const ConvGeom& g, int y0, int x0, int hp, bool inside, int& iy, int& ix)
{
    iy = y0 + hp / HW; ix = x0 + hp % HW;
    return inside && iy >= 0 && iy < g.H && ix >= 0 && ix < g.W;
}

// channel c of input pixel (b, iy, ix)
__device__ __forceinline__ const float* conv_in_ptr(const ConvGeom& g, int b, int iy, int ix, int c)
{
    return g.in + (((int64_t)b * g.H + iy) * g.W + ix) * g.Cin + c;
}

// four channels of a pixel, or zeros (a conditional load) ...
__device__ __forceinline__ float4 conv_load4(const ConvGeom& g, bool ok, int b, int iy, int ix, int c)
{
    return ok ? *reinterpret_cast<const float4*>(conv_in_ptr(g, b, iy, ix, c)) : make_float4(0.f, 0.f, 0.f, 0.f);
}
// ... or read from a block of zeros (an unconditional load: the pipelined kernels keep no branch around a VMEM op)
__device__ __forceinline__ float4 conv_load4(const ConvGeom& g, bool ok, int b, int iy, int ix, int c, const float* zero)
{
    return *reinterpret_cast<const float4*>(ok ? conv_in_ptr(g, b, iy, ix, c) : zero);
}

// ------------------------------------------------------------------ device: epilogues over f32x16 acc[NI][NJ]
// v = acc * scale + shift, ReLU (NaN propagates, like torch.relu), NHWC store inside the channel window
// [coff, coff + Cout) of an ldc-wide pixel.  A wave owns NI x NJ fragments of 32 rows x 32 channels; nw = its first
// channel, lane & 31 = the channel within a fragment.  NULL_SCALE: scale may be null (f32, bf16x6; the f16x3 kernels
// get no test).
//
// 8 x 16 patch layout (TH x TW pixels, row m of the tile = pixel (m / TW, m % TW)); wm = the wave's row of NI fragments.
// MODE 1: tile pixels are input pixels, tap0 the output phase: oy = 2 y + (tap0 >> 1), ox = 2 x + (tap0 & 1).
// GAP (fused global average pooling, gap != null): one partial per (workgroup, wave row) and channel in a fixed order --
// the lane's rows in i, r order, then the other half of the fragment -- for gap_parts_reduce_kernel.
template <int MODE, int TH, int TW, int NI, int NJ, bool NULL_SCALE, bool GAP>
__device__ __forceinline__ void conv_store_patch(const ConvGeom& g, const f32x16 (&acc)[NI][NJ], int b, int ty, int tx, int wm,
                                                 int nw, int tap0, int lane, float* gap = nullptr, int gap_parts = 0)
{
    const int fr = lane & 31, fh = lane >> 5;
    const int MH = MODE == 0 ? g.OH : g.H, MW = MODE == 0 ? g.OW : g.W;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int n = nw + j * 32 + fr;
        if (n >= g.Cout) continue;
        const float sc = NULL_SCALE ? (g.scale ? g.scale[n] : 1.0f) : g.scale[n];
        const float sh = g.shift ? g.shift[n] : 0.0f;
        float gsum = 0.f;                                             // this lane's column: sum of the values it stores
#pragma unroll
        for (int i = 0; i < NI; ++i) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = wm * (32 * NI) + i * 32 + mfma32_crow(r, fh);
                const int y = ty * TH + m / TW, x = tx * TW + m % TW;
                if (y >= MH || x >= MW) continue;
                float v = acc[i][j][r] * sc + sh;
                if (g.relu) v = v <= 0.f ? 0.f : v;                   // NaN propagates, like torch.relu
                int oy = y, ox = x;
                if (MODE == 1) { oy = 2 * y + (tap0 >> 1); ox = 2 * x + (tap0 & 1); }
                g.out[(((int64_t)b * g.OH + oy) * g.OW + ox) * g.ldc + g.coff + n] = v;
                if (GAP) gsum += v;
            }
        }
        if (GAP && gap) {
            gsum += __shfl_xor(gsum, 32);
            if (fh == 0) {
                const int part = (((ty * g.tiles_x + tx) * (MODE == 1 ? 4 : 1) + tap0) << 1) + wm;
                gap[((int64_t)b * gap_parts + part) * g.ldc + g.coff + n] = gsum;
            }
        }
    }
}

// 4 x 32 row layout (the 3x3 halo kernels): fragment i of the wave is image row ty * TH + row0 + i, fragment row = column.
// NCHECK: channel tiles may reach past Cout
template <int TH, int TW, int NI, int NJ, bool NULL_SCALE, bool NCHECK = true>
__device__ __forceinline__ void conv_store_rows(const ConvGeom& g, const f32x16 (&acc)[NI][NJ], int b, int ty, int tx, int row0,
                                                int nw, int lane)
{
    const int fr = lane & 31, fh = lane >> 5;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int n = nw + j * 32 + fr;
        if (NCHECK && n >= g.Cout) continue;
        const float sc = NULL_SCALE ? (g.scale ? g.scale[n] : 1.0f) : g.scale[n];
        const float sh = g.shift ? g.shift[n] : 0.0f;
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int y = ty * TH + row0 + i;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int x = tx * TW + mfma32_crow(r, fh);
                if (y >= g.OH || x >= g.OW) continue;
                float v = acc[i][j][r] * sc + sh;
                if (g.relu) v = v <= 0.f ? 0.f : v;                   // NaN propagates, like torch.relu
                g.out[(((int64_t)b * g.OH + y) * g.OW + x) * g.ldc + g.coff + n] = v;
            }
        }
    }
}

// ------------------------------------------------------------------ device: column reduce of the two GAP forms
// out[b][c] = (sum of the Q rows of C floats of image b, ascending) / div; 64-thread blocks over the channels, grid.y = B
__device__ __forceinline__ void gap_cols_reduce(const float* __restrict__ rows, int Q, int C, float div, float* __restrict__ out)
{
    const int b = blockIdx.y, c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    float s = 0.f;
#pragma unroll 16
    for (int q = 0; q < Q; ++q) s += rows[((int64_t)b * Q + q) * C + c];   // loads run ahead, adds stay in order
    out[(int64_t)b * C + c] = s / div;
}
