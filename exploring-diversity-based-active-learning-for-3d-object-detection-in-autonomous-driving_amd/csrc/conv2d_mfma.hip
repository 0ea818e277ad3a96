// Dense 2-D convolution for the SECOND-style neck and the anchor head as an
// implicit GEMM on the fp32-input matrix cores of gfx950
// (v_mfma_f32_32x32x2_f32: exact f32 products, f32 accumulate, 64 FLOP/clk/SIMD).
//
// Reference layers (det3d/models/necks/rpn.py:124-159, bbox_heads/mg_head.py:215-231):
//   ZeroPad2d(1)+Conv2d(3x3, stride 1|2) / Conv2d(3x3, pad 1) / Conv2d(1x1) /
//   ConvTranspose2d(2x2, stride 2), each followed by eval BatchNorm2d(eps 1e-3)+ReLU
//   (neck) or a bias (head).  BN is folded to per-channel scale/shift and applied in
//   the epilogue together with the ReLU, so activations make one HBM round trip.
//
// Layout: activations NHWC f32 (pixel-major, channels contiguous); weights
// [Cout][tap][Cin] so both GEMM operands are "row x contiguous-K".
// Tiling: 128 output pixels (8x16 patch) x 128 output channels per 256-thread
// workgroup; 4 waves as 2x2, each wave 64x64 = 2x2 MFMA tiles (64 accumulator
// VGPRs); K-chunks of 32 channels per tap, register-staged into double-buffered
// LDS tiles padded to 36 floats per row (conflict-free ds_read_b128 fragments).
// The pixel-tile side (parameter block, tile decode, input pixel, epilogue, entry-point checks) is conv2d_tile.h's.
#include "al3d_common.h"
#include "conv2d_tile.h"

#define CV_BM 128
#define CV_BN 128
#define CV_BK 32
#define CV_LD (CV_BK + 4)
#define CV_TH 8
#define CV_TW 16

struct ConvParams : ConvGeom {
    const float* wgt;     // [Cout, taps, Cin]
};

// MODE 0: convolution (ksize x ksize, stride, pad).  MODE 1: ConvTranspose2d 2x2 stride 2
// (blockIdx.z = output phase dy*2+dx; GEMM-M runs over *input* pixels).
template <int MODE>
__global__ __launch_bounds__(256, 2) void conv2d_mfma_kernel(ConvParams p)
{
    __shared__ __attribute__((aligned(16))) float lds[2][2][CV_BM * CV_LD];  // [buf][A|B]
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int wm = wave & 1, wn = wave >> 1;

    // which pixel patch / image
    int tx_, ty_, b;
    conv_tile_decode(blockIdx.x, p.tiles_x, p.tiles_y, tx_, ty_, b);
    const int n0 = blockIdx.y * CV_BN;
    const int taps = MODE == 0 ? p.ksize * p.ksize : 1;
    const int tap0 = MODE == 0 ? 0 : blockIdx.z;  // deconv: fixed weight tap per launch slice

    // staging role: 8 threads per row (8 x float4 = 32 floats), 32 rows per pass, 4 passes
    const int sq = tid & 7, sr = tid >> 3;
    int py[4], px[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int m = sr + 32 * i;
        py[i] = ty_ * CV_TH + m / CV_TW;
        px[i] = tx_ * CV_TW + m % CV_TW;
    }
    const int kchunks = p.Cin / CV_BK;
    const int nsteps = taps * kchunks;

    float4 ra[4], rb[4];
    auto load_step = [&](int step) {
        const int tap = step / kchunks, c0 = (step - tap * kchunks) * CV_BK;
        const int ky = MODE == 0 ? tap / p.ksize : 0, kx = MODE == 0 ? tap % p.ksize : 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            int iy, ix;
            const bool ok = conv_tap_pixel<MODE>(p, py[i], px[i], ky, kx, iy, ix);
            ra[i] = conv_load4(p, ok, b, iy, ix, c0 + 4 * sq);
            const int n = n0 + sr + 32 * i;
            rb[i] = n < p.Cout ? *reinterpret_cast<const float4*>(
                                     p.wgt + ((int64_t)n * (MODE == 0 ? taps : 4) + tap0 + tap) * p.Cin +
                                     c0 + 4 * sq)
                               : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };
    auto store_step = [&](int buf) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = sr + 32 * i;
            *reinterpret_cast<float4*>(&lds[buf][0][row * CV_LD + 4 * sq]) = ra[i];
            *reinterpret_cast<float4*>(&lds[buf][1][row * CV_LD + 4 * sq]) = rb[i];
        }
    };

    f32x16 acc[2][2];
    conv_acc_clear(acc);

    load_step(0);
    store_step(0);
    __syncthreads();
    const int fr = lane & 31, fh = lane >> 5;
    for (int step = 0; step < nsteps; ++step) {
        const int buf = step & 1;
        if (step + 1 < nsteps) load_step(step + 1);
        const float* As = &lds[buf][0][(wm * 64 + fr) * CV_LD + 4 * fh];
        const float* Bs = &lds[buf][1][(wn * 64 + fr) * CV_LD + 4 * fh];
#pragma unroll
        for (int kg = 0; kg < CV_BK / 8; ++kg) {
            const float4 a0 = *reinterpret_cast<const float4*>(As + kg * 8);
            const float4 a1 = *reinterpret_cast<const float4*>(As + 32 * CV_LD + kg * 8);
            const float4 b0 = *reinterpret_cast<const float4*>(Bs + kg * 8);
            const float4 b1 = *reinterpret_cast<const float4*>(Bs + 32 * CV_LD + kg * 8);
            const float av0[4] = {a0.x, a0.y, a0.z, a0.w}, av1[4] = {a1.x, a1.y, a1.z, a1.w};
            const float bv0[4] = {b0.x, b0.y, b0.z, b0.w}, bv1[4] = {b1.x, b1.y, b1.z, b1.w};
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av0[s], bv0[s], acc[0][0], 0, 0, 0);
                acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av0[s], bv1[s], acc[0][1], 0, 0, 0);
                acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av1[s], bv0[s], acc[1][0], 0, 0, 0);
                acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av1[s], bv1[s], acc[1][1], 0, 0, 0);
            }
        }
        if (step + 1 < nsteps) store_step(buf ^ 1);
        __syncthreads();
    }

    conv_store_patch<MODE, CV_TH, CV_TW, 2, 2, true, false>(p, acc, b, ty_, tx_, wm, n0 + wn * 64, tap0, lane);
}

extern "C" int al3d_conv2d_nhwc_f32(const float* in, const float* wgt, const float* scale,
                                    const float* shift, float* out, int B, int H, int W, int Cin,
                                    int Cout, int ksize, int stride, int pad, int ldc, int coff,
                                    int relu, void* stream)
{
    ConvParams p;
    p.wgt = wgt;
    int rc = conv_geom_build(p, "al3d_conv2d_nhwc_f32", false, CV_TH, CV_TW, CV_BK, false, in, wgt, scale, shift, out, B, H, W,
                             Cin, Cout, ksize, stride, pad, ldc, coff, relu);
    if (rc) return rc;
    dim3 grid((unsigned)(p.tiles_x * p.tiles_y * B), (unsigned)al3d_cdiv(Cout, CV_BN), 1);
    hipLaunchKernelGGL(conv2d_mfma_kernel<0>, grid, dim3(256), 0, (hipStream_t)stream, p);
    AL3D_CHECK_LAUNCH("conv2d_mfma_kernel<conv>");
    return AL3D_OK;
}

extern "C" int al3d_deconv2x2_nhwc_f32(const float* in, const float* wgt, const float* scale,
                                       const float* shift, float* out, int B, int H, int W, int Cin,
                                       int Cout, int ldc, int coff, int relu, void* stream)
{
    ConvParams p;
    p.wgt = wgt;
    int rc = conv_geom_build(p, "al3d_deconv2x2_nhwc_f32", true, CV_TH, CV_TW, CV_BK, false, in, wgt, scale, shift, out, B, H, W,
                             Cin, Cout, 2, 2, 0, ldc, coff, relu);
    if (rc) return rc;
    dim3 grid((unsigned)(p.tiles_x * p.tiles_y * B), (unsigned)al3d_cdiv(Cout, CV_BN), 4);
    hipLaunchKernelGGL(conv2d_mfma_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, p);
    AL3D_CHECK_LAUNCH("conv2d_mfma_kernel<deconv>");
    return AL3D_OK;
}

// ------------------------------------------------------------------ BEV embedding
// x.mean(-1).mean(-1) of the NCHW neck output == per channel: mean over W, then mean
// over H (feature_selector.py:68-71).  NHWC input [B,H,W,C] -> [B,C].  One workgroup
// per (image, 64-channel slab); rows are reduced left-to-right, then top-to-bottom.
// stage 1: one workgroup per image row (b, y): rowmean[b][y][c] = (sum_x x[b,y,x,c]) / W,
// lanes run over channels so every load is a full 1 KiB line; HBM-bound (reads the map once).
__global__ __launch_bounds__(256) void gap_rows_kernel(const float* __restrict__ x, int W, int C,
                                                       float* __restrict__ rowmean)
{
    const int64_t by = blockIdx.x;
    const float* row = x + by * W * C;
    for (int c = threadIdx.x; c < C; c += 256) {
        float s = 0.f;
        for (int xx = 0; xx < W; ++xx) s += row[(int64_t)xx * C + c];
        rowmean[by * C + c] = s / (float)W;
    }
}

// same reduction with 16-byte loads: a thread owns four consecutive channels (C % 4 == 0), so a row of
// C = 512 channels is one 128-lane load per pixel instead of two 256-lane ones; every channel is
// still summed left to right in its own accumulator (bit-identical to the scalar kernel).
__global__ __launch_bounds__(256) void gap_rows_vec4_kernel(const float* __restrict__ x, int W, int C, int rows,
                                                            float* __restrict__ rowmean)
{
    const int c4 = C >> 2;                                   // float4 lanes per pixel
    const int per_block = 256 / c4 > 0 ? 256 / c4 : 1;      // image rows handled by one workgroup
    const int sub = threadIdx.x / c4, lane = threadIdx.x % c4;
    const int64_t by = (int64_t)blockIdx.x * per_block + sub;
    if (sub >= per_block || by >= rows) return;
    const float4* row = reinterpret_cast<const float4*>(x + by * W * C) + lane;
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 8
    for (int xx = 0; xx < W; ++xx) {
        const float4 v = row[(int64_t)xx * c4];
        s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
    const float w = (float)W;
    reinterpret_cast<float4*>(rowmean + by * C)[lane] = make_float4(s.x / w, s.y / w, s.z / w, s.w / w);
}

// stage 2: out[b][c] = (sum_y rowmean[b][y][c]) / H, top to bottom (64-thread blocks: more of them in flight)
__global__ __launch_bounds__(64) void gap_cols_kernel(const float* __restrict__ rowmean, int H, int C,
                                                       float* __restrict__ out)
{
    gap_cols_reduce(rowmean, H, C, (float)H, out);
}

extern "C" int64_t al3d_gap_workspace_bytes(int B, int H, int C) { return (int64_t)B * H * C * 4; }

extern "C" int al3d_gap_nhwc_f32(const float* x, int B, int H, int W, int C, float* out,
                                 void* workspace, void* stream)
{
    AL3D_REQUIRE(x && out && workspace, "al3d_gap_nhwc_f32: null pointer");
    AL3D_REQUIRE(B >= 1 && H >= 1 && W >= 1 && C >= 1, "al3d_gap_nhwc_f32: bad shape");
    float* rowmean = (float*)workspace;
    if (C % 4 == 0 && C / 4 <= 256 && ((uintptr_t)x & 15) == 0 && ((uintptr_t)workspace & 15) == 0) {
        const int per_block = 256 / (C / 4);
        hipLaunchKernelGGL(gap_rows_vec4_kernel, dim3((unsigned)al3d_cdiv((int64_t)B * H, per_block)), dim3(256), 0,
                           (hipStream_t)stream, x, W, C, B * H, rowmean);
    } else {
        hipLaunchKernelGGL(gap_rows_kernel, dim3((unsigned)(B * H)), dim3(256), 0, (hipStream_t)stream, x, W, C,
                           rowmean);
    }
    hipLaunchKernelGGL(gap_cols_kernel, dim3((unsigned)al3d_cdiv(C, 64), (unsigned)B), dim3(64), 0,
                       (hipStream_t)stream, rowmean, H, C, out);
    AL3D_CHECK_LAUNCH("gap_kernel");
    return AL3D_OK;
}
