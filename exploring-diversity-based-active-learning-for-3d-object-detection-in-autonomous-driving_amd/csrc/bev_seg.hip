// Kernels of BEVFusion's BEV map segmentation head (bevfusion/mmdet3d/models/heads/segm/vanilla.py:47-138).
//
//   bev_grid_resample_kernel   BEVGridTransform.forward: F.grid_sample(bilinear, zeros, align_corners = False) on the
//                              axis-aligned grid the class builds.  The grid is a meshgrid of two coordinate vectors, so the
//                              sample is separable: the host hands over, per output row and per output column, the two source
//                              indices and the two weights; the kernel does the four-term blend.
//   seg_classify_kernel        the classifier's last Conv2d(C, K, 1) with bias + torch.sigmoid, and per frame and class
//   seg_reduce_kernel          the summed binary entropy and the count of pixels with p > 0.5.
//
// Both are bandwidth-bound (at the workload's size the resample reads 16.8 MB and writes 41 MB per frame, the classifier
// reads 41 MB and writes 1 MB), so lanes run along channels with 16-byte loads, nothing is read twice from memory and
// there are no atomics.
//
// RESAMPLE.  A thread owns four channels of one output pixel; consecutive threads are consecutive channel quads, then
// consecutive output columns, so a wave covers whole pixels (C = 256: one 1 KB row per wave) and its four source rows
// are contiguous 1 KB reads.  The output row and the frame come from the grid, so the row's table entries are scalar
// loads; a column's index pair and weight pair are one 8-byte load each.  Blend, every operation rounded to f32 on its own (the file is built without contraction):
//     out = r0 * (c0 * v00 + c1 * v01) + r1 * (c0 * v10 + c1 * v11)
// with (r0, r1) the row weights, (c0, c1) the column weights, v_ij the source pixel (row index i, column index j).  A
// source index outside [0, size) contributes zero: its value is replaced by 0, not multiplied by a zero weight (so a padded
// output is exactly 0 whatever the map holds, as in torch).  The kernel tests every index against the map's size itself
// and loads at the index clamped into the map, so no table can make it read outside.
//
// CLASSIFY.  A workgroup of four waves owns 256 consecutive pixels of one frame, a wave 64 of them.  The weights, zero-
// padded to KP = 4, 8 or 16 classes, sit in LDS.  Eight lanes share a pixel (lane = 8 * p + q): lane q reads the channel
// quads q, q + 8, q + 16, ... of its pixel -- one 128-byte line per pixel and load -- and keeps one f32 FMA chain per class,
//     acc = fma(x[c], w[k][c], acc)   over its channels c in ascending order, from acc = 0;
// the eight chains of a pixel are then added as ((a0 + a1) + (a2 + a3)) + ((a4 + a5) + (a6 + a7)) (an xor butterfly over
// q: 1, 2, 4), and the bias is added last.  The 64 x KP logits of the wave go through LDS so that lane = pixel for the
// epilogue: p = 1 / (1 + expf(-z)), a 256-byte store per class into prob [N][K][H][W], the entropy
// -(p logf(p) + (1 - p) logf(1 - p)) (exactly 0 where p is 0 or 1) and p > 0.5.  Reductions, in a fixed order so that two
// runs give the same bits: the wave's 64 entropies by an xor butterfly (32, 16, 8, 4, 2, 1), the four waves in ascending
// order into the workgroup's partial, and seg_reduce_kernel adds the partials of a frame: 16 interleaved slots, each in
// ascending workgroup order, then the slots in ascending order.
#include "al3d_common.h"
#include "al3d_select.h"

// ------------------------------------------------------------------ BEVGridTransform
__global__ __launch_bounds__(256) void bev_grid_resample_kernel(const float* __restrict__ src, int h, int w, int C,
                                                                const int2* __restrict__ row_idx, const float2* __restrict__ row_w,
                                                                const int2* __restrict__ col_idx, const float2* __restrict__ col_w,
                                                                int H, int W, int swapped, float* __restrict__ out)
{
    const int CQ = C >> 2;
    const int t = blockIdx.x * 256 + threadIdx.x;          // (output column, channel quad) of this row
    if (t >= W * CQ) return;
    const int x = t / CQ, c = (t - x * CQ) * 4;
    const int y = blockIdx.y, n = blockIdx.z;               // uniform: the row's table entries are scalar loads
    const int2 yi = row_idx[y], xi = col_idx[x];
    const float2 r = row_w[y], cw = col_w[x];
    const bool iy0 = (unsigned)yi.x < (unsigned)h, iy1 = (unsigned)yi.y < (unsigned)h;
    const bool ix0 = (unsigned)xi.x < (unsigned)w, ix1 = (unsigned)xi.y < (unsigned)w;
    const float* b = src + (int64_t)n * h * w * C + c;
    // four unconditional loads at indices clamped into the map, issued together; an outside tap's value is then dropped
    const int y0 = min(max(yi.x, 0), h - 1), y1 = min(max(yi.y, 0), h - 1);
    const int x0 = min(max(xi.x, 0), w - 1), x1 = min(max(xi.y, 0), w - 1);
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 v00 = *reinterpret_cast<const float4*>(b + ((int64_t)y0 * w + x0) * C);
    float4 v01 = *reinterpret_cast<const float4*>(b + ((int64_t)y0 * w + x1) * C);
    float4 v10 = *reinterpret_cast<const float4*>(b + ((int64_t)y1 * w + x0) * C);
    float4 v11 = *reinterpret_cast<const float4*>(b + ((int64_t)y1 * w + x1) * C);
    if (!(iy0 && ix0)) v00 = zero;
    if (!(iy0 && ix1)) v01 = zero;
    if (!(iy1 && ix0)) v10 = zero;
    if (!(iy1 && ix1)) v11 = zero;
    const float r0 = r.x, r1 = r.y, c0 = cw.x, c1 = cw.y;
    float4 v;
    v.x = r0 * (c0 * v00.x + c1 * v01.x) + r1 * (c0 * v10.x + c1 * v11.x);
    v.y = r0 * (c0 * v00.y + c1 * v01.y) + r1 * (c0 * v10.y + c1 * v11.y);
    v.z = r0 * (c0 * v00.z + c1 * v01.z) + r1 * (c0 * v10.z + c1 * v11.z);
    v.w = r0 * (c0 * v00.w + c1 * v01.w) + r1 * (c0 * v10.w + c1 * v11.w);
    const int64_t opx = swapped ? ((int64_t)n * W + x) * H + y : ((int64_t)n * H + y) * W + x;
    *reinterpret_cast<float4*>(out + opx * C + c) = v;
}

extern "C" int al3d_bev_grid_resample_nhwc_f32(const float* src, int N, int h, int w, int C, const int* row_idx,
                                               const float* row_w, const int* col_idx, const float* col_w, int H, int W,
                                               int out_hw_swapped, float* out, void* stream)
{
    AL3D_REQUIRE(src && out && row_idx && row_w && col_idx && col_w, "al3d_bev_grid_resample_nhwc_f32: null pointer");
    AL3D_REQUIRE(N >= 1 && h >= 1 && w >= 1 && H >= 1 && W >= 1,
                 "al3d_bev_grid_resample_nhwc_f32: non-positive size (N=%d, %d x %d -> %d x %d)", N, h, w, H, W);
    AL3D_REQUIRE(C >= 4 && C % 4 == 0, "al3d_bev_grid_resample_nhwc_f32: C=%d must be a positive multiple of 4", C);
    AL3D_REQUIRE((((uintptr_t)src | (uintptr_t)out) & 15) == 0, "al3d_bev_grid_resample_nhwc_f32: 16-byte aligned maps");
    AL3D_REQUIRE((((uintptr_t)row_idx | (uintptr_t)row_w | (uintptr_t)col_idx | (uintptr_t)col_w) & 7) == 0,
                 "al3d_bev_grid_resample_nhwc_f32: 8-byte aligned tables");
    AL3D_REQUIRE(out_hw_swapped == 0 || out_hw_swapped == 1, "al3d_bev_grid_resample_nhwc_f32: out_hw_swapped=%d is not 0 or 1",
                 out_hw_swapped);
    const int64_t row = (int64_t)W * (C / 4);                // threads of an output row
    AL3D_REQUIRE(row < ((int64_t)1 << 30) && H <= 65535 && N <= 65535 && (int64_t)h * w * C < ((int64_t)1 << 40),
                 "al3d_bev_grid_resample_nhwc_f32: map too large");
    hipLaunchKernelGGL(bev_grid_resample_kernel, dim3((unsigned)al3d_cdiv(row, 256), (unsigned)H, (unsigned)N), dim3(256), 0,
                       (hipStream_t)stream, src, h, w, C, (const int2*)row_idx, (const float2*)row_w, (const int2*)col_idx,
                       (const float2*)col_w, H, W, out_hw_swapped, out);
    AL3D_CHECK_LAUNCH("bev_grid_resample_kernel");
    return AL3D_OK;
}

// ------------------------------------------------------------------ Conv2d(C, K, 1) + sigmoid + per-frame reductions
#define SEG_TILE 256            // pixels of a workgroup (64 per wave)
#define SEG_KMAX 16

struct SegPartial {             // one workgroup's share of a frame's reductions
    float entropy[SEG_KMAX];
    int area[SEG_KMAX];
};

static inline int seg_kpad(int K) { return K <= 4 ? 4 : (K <= 8 ? 8 : 16); }
static inline int64_t seg_tiles(int H, int W) { return al3d_cdiv((int64_t)H * W, SEG_TILE); }

template <int KP>
__global__ __launch_bounds__(256) void seg_classify_kernel(const float* __restrict__ in, const float* __restrict__ wgt,
                                                           const float* __restrict__ bias, int HW, int C, int K,
                                                           float* __restrict__ prob, SegPartial* __restrict__ partial)
{
    extern __shared__ __attribute__((aligned(16))) float seg_lds[];
    float* e_s = seg_lds;                                  // [4 waves][16] entropy sums
    int* c_s = reinterpret_cast<int*>(seg_lds + 64);       // [4 waves][16] counts
    float* w_s = seg_lds + 128;                            // [KP][C], rows K.. zero
    float* z_s = w_s + KP * C;                             // [4 waves][KP][64]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int CQ = C >> 2;
    const int n = blockIdx.y;
    for (int i = threadIdx.x; i < KP * CQ; i += 256) {
        const int k = i / CQ;
        reinterpret_cast<float4*>(w_s)[i] =
            k < K ? reinterpret_cast<const float4*>(wgt)[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    __syncthreads();

    const int q = lane & 7, p = lane >> 3;
    const int base = blockIdx.x * SEG_TILE + wave * 64;   // this wave's first pixel of the frame
    float* zw = z_s + wave * KP * 64;
    const float* frame = in + (int64_t)n * HW * C;
#pragma unroll 1
    for (int it = 0; it < 4; ++it) {
        const int la = it * 16 + p, lb = la + 8;           // the lane's two pixels of this round (wave-local)
        const bool va = base + la < HW, vb = base + lb < HW;
        const float4* xa = reinterpret_cast<const float4*>(frame + (int64_t)(base + la) * C);
        const float4* xb = reinterpret_cast<const float4*>(frame + (int64_t)(base + lb) * C);
        constexpr int UNROLL = KP == 16 ? 1 : 2;            // 16 classes: 64 weight registers per step already
        float acc[2][KP];
#pragma unroll
        for (int k = 0; k < KP; ++k) acc[0][k] = acc[1][k] = 0.f;
#pragma unroll UNROLL
        for (int cq = q; cq < CQ; cq += 8) {
            const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
            const float4 a = va ? xa[cq] : zero, b = vb ? xb[cq] : zero;
#pragma unroll
            for (int k = 0; k < KP; ++k) {
                const float4 wv = reinterpret_cast<const float4*>(w_s + k * C)[cq];
                acc[0][k] = __builtin_fmaf(a.x, wv.x, acc[0][k]);
                acc[0][k] = __builtin_fmaf(a.y, wv.y, acc[0][k]);
                acc[0][k] = __builtin_fmaf(a.z, wv.z, acc[0][k]);
                acc[0][k] = __builtin_fmaf(a.w, wv.w, acc[0][k]);
                acc[1][k] = __builtin_fmaf(b.x, wv.x, acc[1][k]);
                acc[1][k] = __builtin_fmaf(b.y, wv.y, acc[1][k]);
                acc[1][k] = __builtin_fmaf(b.z, wv.z, acc[1][k]);
                acc[1][k] = __builtin_fmaf(b.w, wv.w, acc[1][k]);
            }
        }
#pragma unroll
        for (int k = 0; k < KP; ++k) {
#pragma unroll
            for (int g = 0; g < 2; ++g) {
                float s = acc[g][k];
                s = s + __shfl_xor(s, 1);
                s = s + __shfl_xor(s, 2);
                s = s + __shfl_xor(s, 4);
                if (q == (k & 7)) zw[k * 64 + (g ? lb : la)] = s;
            }
        }
    }
    __syncthreads();

    // lane = pixel
    const int px = base + lane;
    const bool valid = px < HW;
#pragma unroll
    for (int k = 0; k < KP; ++k) {
        if (k < K) {
            const float z = zw[k * 64 + lane] + bias[k];
            const float pr = al3d_sigmoid(z);
            if (valid) prob[((int64_t)n * K + k) * HW + px] = pr;
            if (partial) {
                float e = 0.f;
                if (valid && pr > 0.f && pr < 1.f) {
                    const float o = 1.0f - pr;
                    e = -(pr * logf(pr) + o * logf(o));
                }
#pragma unroll
                for (int m = 32; m >= 1; m >>= 1) e = e + __shfl_xor(e, m);
                const int cnt = __popcll(__ballot(valid && pr > 0.5f));
                if (lane == 0) {
                    e_s[wave * SEG_KMAX + k] = e;
                    c_s[wave * SEG_KMAX + k] = cnt;
                }
            }
        }
    }
    if (!partial) return;                                   // uniform over the grid
    __syncthreads();
    if (threadIdx.x < SEG_KMAX) {
        const int k = threadIdx.x;
        float e = 0.f;
        int c = 0;
        if (k < K) {
            e = ((e_s[k] + e_s[SEG_KMAX + k]) + e_s[2 * SEG_KMAX + k]) + e_s[3 * SEG_KMAX + k];
            c = c_s[k] + c_s[SEG_KMAX + k] + c_s[2 * SEG_KMAX + k] + c_s[3 * SEG_KMAX + k];
        }
        SegPartial* dst = partial + (int64_t)n * gridDim.x + blockIdx.x;
        dst->entropy[k] = e;
        dst->area[k] = c;
    }
}

// One workgroup per frame: thread = (slot, class); slot s of 16 adds the partials of the workgroups s, s + 16, ... in
// ascending order, then the 16 slots are added in ascending order.
__global__ __launch_bounds__(256) void seg_reduce_kernel(const SegPartial* __restrict__ partial, int tiles, int K,
                                                         float* __restrict__ entropy_sum, int* __restrict__ area)
{
    __shared__ float e_s[16][SEG_KMAX];
    __shared__ int c_s[16][SEG_KMAX];
    const int k = threadIdx.x & 15, slot = threadIdx.x >> 4, n = blockIdx.x;
    const SegPartial* src = partial + (int64_t)n * tiles;
    float e = 0.f;
    int c = 0;
    for (int i = slot; i < tiles; i += 16) {
        e = e + src[i].entropy[k];
        c += src[i].area[k];
    }
    e_s[slot][k] = e;
    c_s[slot][k] = c;
    __syncthreads();
    if (threadIdx.x < K) {
        e = 0.f;
        c = 0;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            e = e + e_s[i][k];
            c += c_s[i][k];
        }
        if (entropy_sum) entropy_sum[n * K + k] = e;
        if (area) area[n * K + k] = c;
    }
}

extern "C" int64_t al3d_seg_classify_workspace_bytes(int N, int H, int W)
{
    if (N < 1 || H < 1 || W < 1) return 0;
    return (int64_t)N * seg_tiles(H, W) * (int64_t)sizeof(SegPartial);
}

extern "C" int al3d_seg_classify_f32(const float* in, const float* w, const float* b, int N, int H, int W, int C, int K,
                                     float* prob, float* entropy_sum, int* area, void* workspace, void* stream)
{
    AL3D_REQUIRE(in && w && b && prob, "al3d_seg_classify_f32: null pointer");
    AL3D_REQUIRE(N >= 1 && H >= 1 && W >= 1, "al3d_seg_classify_f32: non-positive size (N=%d, %d x %d)", N, H, W);
    AL3D_REQUIRE(C >= 4 && C % 4 == 0, "al3d_seg_classify_f32: C=%d must be a positive multiple of 4", C);
    AL3D_REQUIRE(K >= 1 && K <= SEG_KMAX, "al3d_seg_classify_f32: K=%d is outside [1, %d]", K, SEG_KMAX);
    AL3D_REQUIRE((((uintptr_t)in | (uintptr_t)w) & 15) == 0, "al3d_seg_classify_f32: 16-byte aligned map and weights");
    AL3D_REQUIRE((((uintptr_t)b | (uintptr_t)prob | (uintptr_t)entropy_sum | (uintptr_t)area) & 3) == 0,
                 "al3d_seg_classify_f32: 4-byte aligned bias and outputs");
    const bool stats = entropy_sum || area;
    AL3D_REQUIRE(!stats || (workspace && ((uintptr_t)workspace & 3) == 0),
                 "al3d_seg_classify_f32: the reductions need a 4-byte aligned workspace of al3d_seg_classify_workspace_bytes");
    const int KP = seg_kpad(K);
    const int64_t lds = 512 + (int64_t)KP * (C + 256) * 4;     // reductions, weights, the waves' logits
    AL3D_REQUIRE(lds <= 65536, "al3d_seg_classify_f32: K=%d classes (padded to %d) x C=%d channels do not fit in LDS", K, KP, C);
    AL3D_REQUIRE((int64_t)H * W < ((int64_t)1 << 30) && N <= 65535, "al3d_seg_classify_f32: map too large");
    const int HW = H * W;
    const int tiles = (int)seg_tiles(H, W);
    SegPartial* partial = stats ? (SegPartial*)workspace : nullptr;
    const dim3 grid((unsigned)tiles, (unsigned)N);
#define SEG_LAUNCH(KPAD)                                                                                                  \
    hipLaunchKernelGGL(seg_classify_kernel<KPAD>, grid, dim3(256), (size_t)lds, (hipStream_t)stream, in, w, b, HW, C, K, \
                       prob, partial)
    if (KP == 4) SEG_LAUNCH(4);
    else if (KP == 8) SEG_LAUNCH(8);
    else SEG_LAUNCH(16);
#undef SEG_LAUNCH
    AL3D_CHECK_LAUNCH("seg_classify_kernel");
    if (stats) {
        hipLaunchKernelGGL(seg_reduce_kernel, dim3((unsigned)N), dim3(256), 0, (hipStream_t)stream, partial, tiles, K,
                           entropy_sum, area);
        AL3D_CHECK_LAUNCH("seg_reduce_kernel");
    }
    return AL3D_OK;
}
