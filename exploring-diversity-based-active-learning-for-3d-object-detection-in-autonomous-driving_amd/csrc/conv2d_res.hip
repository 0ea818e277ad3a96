// Kernels of the camera-only BEV decoder (GeneralizedResNet + LSSFPN behind the plain LSS view transform).
//
//   conv3x3_res_f16x3_kernel   3x3 / s1 / p1 convolution + affine + residual + ReLU: conv2 + bn2 + shortcut + ReLU of a
//                              ResNet BasicBlock as one launch, f16x3 arithmetic (al3d_f16x3.h)
//   add_relu_kernel            relu(x + res): the same residual step behind a convolution of the other arithmetics
//   upsample_bilinear_ac_kernel  bilinear resize, align_corners = True (LSSFPN's tail)
//
// The BEV maps of this decoder are small (B = 16: 32 x 32 x 128, 16 x 16 x 256, 16 x 16 x 512 per sample): what counts
// is one launch per block half and a grid that covers the chip, not the peak rate of a 128 x 128 workgroup tile.  So a
// WAVE owns 32 pixels (4 rows x 8 columns) x 32 output channels -- one v_mfma_f32_32x32x16_f16 accumulator, the shape the
// other dense f16x3 kernels use, which is what keeps the result bit-identical to theirs -- and the four waves of a
// workgroup are four channel tiles of the same pixel tile (they read the same activations: vector-L1 hits).  The deepest
// layer, 16 x 16 x 16 x 512, is then 128 pixel tiles x 16 channel tiles = 2,048 waves = two per SIMD on 256 CUs.
// Nothing goes through LDS and there is no barrier: the A fragment is two 16-byte loads per lane straight from the map
// (lane = pixel, k half), split in registers; the B fragments are 16-byte loads from al3d_pack_f16x3_dma's per-step
// images (1 KB contiguous per wave and plane).  Step s + 1 is requested before the products of step s are issued.
// Maps large enough to give every SIMD four waves run two channel tiles per wave (one split feeds both).
//
// Steps run tap-major, 16 input channels at a time, and every accumulator receives xl'*wd, xh*wl, xh*wh in that order:
// the order of conv2d_f16x3_kernel / conv2d_f16x3_dma_kernel.  The epilogue is (acc * scale + shift) + res, then ReLU,
// each operation rounded to f32 on its own (the file is built without contraction).
#include "al3d_common.h"
#include "al3d_f16x3.h"
#include "conv2d_tile.h"

#define R3_TH 4
#define R3_TW 8

struct ConvResParams : ConvGeom {         // 3x3 / s1 / p1: OH, OW = H, W; 4 x 8 pixel tiles; scale required
    const char* wgt;        // al3d_pack_f16x3_dma image: [ceil(Cout/128)][9][Cin/16] stages of 8 KB
    const float* res;       // [B, H, W, ldr] f32
    int ldr, ngroups;
};

__device__ __attribute__((aligned(32))) float g_res_zero[8];       // stays zero: source of out-of-image pixels

template <int NB>
__global__ __launch_bounds__(256) void conv3x3_res_f16x3_kernel(ConvResParams p)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int group = blockIdx.y * 4 + wave;              // this wave's NB channel tiles
    if (group >= p.ngroups) return;                       // wave-uniform; the kernel has no barrier
    const int fr = lane & 31, fh = lane >> 5;
    int tx_, ty_, b;
    conv_tile_decode(blockIdx.x, p.tiles_x, p.tiles_y, tx_, ty_, b);
    const int py = ty_ * R3_TH + (fr >> 3), px = tx_ * R3_TW + (fr & 7);
    const bool live = py < p.H && px < p.W;
    const int kchunks = p.Cin >> 4;
    const int total = 9 * kchunks;
    const int n_base = group * 32 * NB;

    // weight stream: stage (block, tap, chunk) = [2 planes][128 rows][2 halves of 8 f16], half c of row n at c ^ ((n >> 3) & 1)
    const char* wsrc[NB];
#pragma unroll
    for (int j = 0; j < NB; ++j) {
        const int n = n_base + 32 * j + fr, nl = n & 127;
        wsrc[j] = p.wgt + (int64_t)(n >> 7) * total * 8192 + nl * 32 + ((fh ^ ((nl >> 3) & 1)) * 16);
    }

    int ltap = 0, lchunk = 0;                             // cursor of the next step to request
    const float* arow = g_res_zero;
    bool aok = false;
    auto set_tap = [&](int tap) {                         // (its own pixel test: stride and pad are constants here, not p's)
        const int ky = tap / 3, kx = tap - 3 * ky;
        const int iy = py + ky - 1, ix = px + kx - 1;
        aok = live && iy >= 0 && iy < p.H && ix >= 0 && ix < p.W;
        arow = aok ? p.in + (((int64_t)b * p.H + iy) * p.W + ix) * p.Cin + 8 * fh : g_res_zero;
    };
    auto request = [&](float4 (&a)[2], f16x8 (&wh)[NB], f16x8 (&wl)[NB]) {
        const float* src = aok ? arow + lchunk * 16 : g_res_zero;
        a[0] = *reinterpret_cast<const float4*>(src);
        a[1] = *reinterpret_cast<const float4*>(src + 4);
        const int64_t off = (int64_t)(ltap * kchunks + lchunk) * 8192;
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            wh[j] = *reinterpret_cast<const f16x8*>(wsrc[j] + off);
            wl[j] = *reinterpret_cast<const f16x8*>(wsrc[j] + off + 4096);
        }
        if (++lchunk == kchunks) { lchunk = 0; if (++ltap < 9) set_tap(ltap); }
    };

    f32x16 acc[1][NB];
    conv_acc_clear(acc);

    float4 a_cur[2], a_nxt[2];
    f16x8 wh_cur[NB], wl_cur[NB], wh_nxt[NB], wl_nxt[NB];
    set_tap(0);
    request(a_cur, wh_cur, wl_cur);
    for (int s = 0; s < total; ++s) {
        if (s + 1 < total) request(a_nxt, wh_nxt, wl_nxt);
        f16x8 ah, al;
        f3_split8(a_cur[0], a_cur[1], ah, al);
#pragma unroll
        for (int j = 0; j < NB; ++j) f3_mac3(ah, al, wh_cur[j], wl_cur[j], f3_lift_down(wh_cur[j]), acc[0][j]);
        a_cur[0] = a_nxt[0]; a_cur[1] = a_nxt[1];
#pragma unroll
        for (int j = 0; j < NB; ++j) { wh_cur[j] = wh_nxt[j]; wl_cur[j] = wl_nxt[j]; }
    }

    // C layout of the 32 x 32 product: lane column fr = channel, register r = pixel (r & 3) + 8 (r >> 2) + 4 fh.  Private to
    // this kernel: the residual is added between the affine and the ReLU
#pragma unroll
    for (int j = 0; j < NB; ++j) {
        const int n = n_base + 32 * j + fr;
        const float sc = p.scale[n];
        const float sh = p.shift ? p.shift[n] : 0.0f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = f3_crow(r, fh);
            const int y = ty_ * R3_TH + (m >> 3), x = tx_ * R3_TW + (m & 7);
            if (y >= p.H || x >= p.W) continue;
            const int64_t pix = ((int64_t)b * p.H + y) * p.W + x;
            float v = acc[0][j][r] * sc + sh;
            v = v + p.res[pix * p.ldr + n];
            if (p.relu) v = v <= 0.f ? 0.f : v;                             // NaN propagates, like torch.relu
            p.out[pix * p.ldc + p.coff + n] = v;
        }
    }
}

extern "C" int al3d_conv3x3_res_nhwc_f16x3(const float* in, const void* wgt_image, const float* scale, const float* shift,
                                           const float* res, float* out, int B, int H, int W, int Cin, int Cout, int ldr,
                                           int ldc, int coff, int relu, void* stream)
{
    const char* name = "al3d_conv3x3_res_nhwc_f16x3";
    ConvResParams p;
    p.wgt = (const char*)wgt_image; p.res = res; p.ldr = ldr;
    conv_geom_set(p, false, R3_TH, R3_TW, in, scale, shift, out, B, H, W, Cin, Cout, 3, 1, 1, ldc, coff, relu);
    int rc = conv_geom_check(p, wgt_image, name, 16, true);
    if (rc) return rc;
    AL3D_REQUIRE(res, "%s: null residual (the plain convolution is al3d_conv2d_nhwc_f16x3_dma)", name);
    AL3D_REQUIRE(Cout % 32 == 0, "%s: Cout=%d must be a multiple of 32", name, Cout);
    AL3D_REQUIRE(ldr >= Cout, "%s: residual row stride ldr=%d is below Cout=%d", name, ldr, Cout);
    const int64_t ntiles = (int64_t)p.tiles_x * p.tiles_y * B;
    AL3D_REQUIRE(ntiles < ((int64_t)1 << 31), "%s: map above 2^31 pixel tiles", name);
    // two channel tiles per wave once that still leaves every SIMD of 256 CUs two waves
    const bool two = Cout % 64 == 0 && ntiles * (Cout / 32) >= 4096;
    p.ngroups = Cout / (two ? 64 : 32);
    const dim3 grid((unsigned)ntiles, (unsigned)al3d_cdiv(p.ngroups, 4));
    if (two) hipLaunchKernelGGL(conv3x3_res_f16x3_kernel<2>, grid, dim3(256), 0, (hipStream_t)stream, p);
    else hipLaunchKernelGGL(conv3x3_res_f16x3_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, p);
    AL3D_CHECK_LAUNCH("conv3x3_res_f16x3_kernel");
    return AL3D_OK;
}

// ------------------------------------------------------------------ relu(x + res), four channels per thread
__global__ __launch_bounds__(256) void add_relu_kernel(const float* x, const float* res, float* out,
                                                       int64_t total, int CQ, int ldx, int ldr, int ldc, int relu)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const int64_t px = t / CQ;
    const int c = (int)(t - px * CQ) * 4;
    const float4 a = *reinterpret_cast<const float4*>(x + px * ldx + c);
    const float4 r = *reinterpret_cast<const float4*>(res + px * ldr + c);
    float v[4] = {a.x + r.x, a.y + r.y, a.z + r.z, a.w + r.w};
    if (relu) {
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = v[i] <= 0.f ? 0.f : v[i];      // NaN propagates
    }
    *reinterpret_cast<float4*>(out + px * ldc + c) = make_float4(v[0], v[1], v[2], v[3]);
}

extern "C" int al3d_add_relu_nhwc_f32(const float* x, const float* res, float* out, int64_t n_pixels, int C, int ldx, int ldr,
                                      int ldc, int relu, void* stream)
{
    AL3D_REQUIRE(x && res && out, "al3d_add_relu_nhwc_f32: null pointer");
    AL3D_REQUIRE(n_pixels >= 0 && C >= 4 && C % 4 == 0, "al3d_add_relu_nhwc_f32: C=%d must be a positive multiple of 4", C);
    AL3D_REQUIRE(ldx >= C && ldr >= C && ldc >= C && ldx % 4 == 0 && ldr % 4 == 0 && ldc % 4 == 0,
                 "al3d_add_relu_nhwc_f32: row strides (%d, %d, %d) must be multiples of 4 and at least C=%d", ldx, ldr, ldc, C);
    AL3D_REQUIRE((((uintptr_t)x | (uintptr_t)res | (uintptr_t)out) & 15) == 0, "al3d_add_relu_nhwc_f32: 16-byte aligned maps");
    const int64_t total = n_pixels * (C / 4);
    if (total == 0) return AL3D_OK;
    AL3D_REQUIRE(al3d_cdiv(total, 256) < ((int64_t)1 << 31), "al3d_add_relu_nhwc_f32: map too large");
    hipLaunchKernelGGL(add_relu_kernel, dim3((unsigned)al3d_cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, x, res, out,
                       total, C / 4, ldx, ldr, ldc, relu);
    AL3D_CHECK_LAUNCH("add_relu_kernel");
    return AL3D_OK;
}

// ------------------------------------------------------------------ bilinear resize, align_corners = True
// The upsampled half of lss_upsample_cat_kernel<true> (bev_pool.hip) without the lateral copy: source position in f32
// s * o with s = (in - 1) / (out - 1) (0 for a single output row / column), the lower neighbour by truncation, the upper
// one clamped at the border, and the blend h0 (w0 v00 + w1 v01) + h1 (w0 v10 + w1 v11).  A thread owns four channels
// of an output pixel.
__global__ __launch_bounds__(256) void upsample_bilinear_ac_kernel(const float* __restrict__ src, int64_t total, int H, int W, int h,
                                                                   int w, int C, float sh, float sw, float* __restrict__ out)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const int CQ = C >> 2;
    const int c = (int)(t % CQ) * 4;
    const int64_t px = t / CQ;
    const int x = (int)(px % W), y = (int)((px / W) % H);
    const int64_t n = px / ((int64_t)W * H);
    const float yr = sh * (float)y, xr = sw * (float)x;
    const int y0 = (int)yr, x0 = (int)xr;
    const int yp = y0 < h - 1 ? 1 : 0, xp = x0 < w - 1 ? 1 : 0;
    const float ly = yr - (float)y0, lx = xr - (float)x0, hy = 1.0f - ly, hx = 1.0f - lx;
    const float* b = src + ((n * h + y0) * w + x0) * C + c;
    const float4 v00 = *reinterpret_cast<const float4*>(b), v01 = *reinterpret_cast<const float4*>(b + (int64_t)xp * C);
    const float4 v10 = *reinterpret_cast<const float4*>(b + (int64_t)yp * w * C);
    const float4 v11 = *reinterpret_cast<const float4*>(b + ((int64_t)yp * w + xp) * C);
    float4 v;
    v.x = hy * (hx * v00.x + lx * v01.x) + ly * (hx * v10.x + lx * v11.x);
    v.y = hy * (hx * v00.y + lx * v01.y) + ly * (hx * v10.y + lx * v11.y);
    v.z = hy * (hx * v00.z + lx * v01.z) + ly * (hx * v10.z + lx * v11.z);
    v.w = hy * (hx * v00.w + lx * v01.w) + ly * (hx * v10.w + lx * v11.w);
    *reinterpret_cast<float4*>(out + px * C + c) = v;
}

extern "C" int al3d_upsample_bilinear_ac_nhwc_f32(const float* src, int N, int h, int w, int C, int H, int W, float* out,
                                                  void* stream)
{
    AL3D_REQUIRE(src && out, "al3d_upsample_bilinear_ac_nhwc_f32: null pointer");
    AL3D_REQUIRE(N >= 0 && h >= 1 && w >= 1 && H >= 1 && W >= 1 && C >= 4 && C % 4 == 0,
                 "al3d_upsample_bilinear_ac_nhwc_f32: bad shape (C=%d must be a positive multiple of 4)", C);
    AL3D_REQUIRE((((uintptr_t)src | (uintptr_t)out) & 15) == 0, "al3d_upsample_bilinear_ac_nhwc_f32: 16-byte aligned maps");
    const int64_t total = (int64_t)N * H * W * (C / 4);
    if (total == 0) return AL3D_OK;
    AL3D_REQUIRE(al3d_cdiv(total, 256) < ((int64_t)1 << 31), "al3d_upsample_bilinear_ac_nhwc_f32: map too large");
    const float sh = H > 1 ? (float)(h - 1) / (float)(H - 1) : 0.f, sw = W > 1 ? (float)(w - 1) / (float)(W - 1) : 0.f;
    hipLaunchKernelGGL(upsample_bilinear_ac_kernel, dim3((unsigned)al3d_cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, src,
                       total, H, W, h, w, C, sh, sw, out);
    AL3D_CHECK_LAUNCH("upsample_bilinear_ac_kernel");
    return AL3D_OK;
}
