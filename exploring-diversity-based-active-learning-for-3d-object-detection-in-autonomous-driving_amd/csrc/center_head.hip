// CenterPoint head on device: the grouped last convolutions of the separate heads and the whole post-processing
// (per-class top-K, cross-class top-K, gather + decode, the two filters, rotated or circle NMS, merge).
//
// Reference: CenterHead.get_bboxes / get_task_detections (bevfusion/mmdet3d/models/heads/bbox/centerpoint.py:637-757,
// 759-884), CenterPointBBoxCoder._topk / decode (core/bbox/coders/centerpoint_bbox_coders.py:62-100,121-225),
// xywhr2xyxyr (core/bbox/structures/utils.py:71-89), nms_gpu (ops/iou3d/iou3d_utils.py:23-48) with iou_bev / nms_kernel
// (ops/iou3d/src/iou3d_kernel.cu:244-250,300-331), circle_nms (core/post_processing/box3d_nms.py:180-219), SeparateHead
// (centerpoint.py:20-125).  The reference runs, per task, two torch.topk, six gathers, a boolean-mask index per sample
// (a host synchronisation each) and an NMS that copies to the host; here a whole-GPU pre-pass writes the sigmoid scores
// as sortable keys and one workgroup per (sample, task) does everything else in LDS, with no host synchronisation.
//
// torch.topk leaves the order of equal scores open.  The tie rule of al3d_select.h decides, on the flat index
// class * D0 * D1 + cell, cell = d0 * D1 + d1 in the map as it is handed to the kernel.
// Comparisons: the coder's score filter is strict (score > threshold, coder :196), its centre range closed (:198-216);
// get_task_detections keeps score >= test score threshold (:818); the rotated NMS suppresses on IoU > nms_thr, strictly
// (iou3d_kernel.cu:326; the anchor head's loop in head_nms.hip uses >=); the circle NMS on squared distance <= radius.
#include "al3d_common.h"
#include "al3d_rbox.h"
#include "al3d_select.h"

#define CT_THREADS 1024
#define CT_MAXK 1024            // max_num <= 1024
#define CT_MAXCAND 2048         // classes of a task x max_num
#define CT_MAXPOST 512
#define CT_MAXCLS 4
#define CT_MAXTASKS 8

struct CenterTask {
    int ncls;
    int heat_off, reg_off, hei_off, dim_off, rot_off, vel_off;      // channel offsets in the head output; reg / vel: -1 = absent
    int key_off;                                                    // first class of the task in the key planes
    int label_off;
    int nms_kind;                                                   // 0 rotate, 1 circle
    float radius;
    float nms_scale[CT_MAXCLS];
};

struct CenterParams {
    const float* hout;          // [B, D0, D1, CH]
    int B, D0, D1, CH, ntasks, sumC;
    int swapped;                // 0: the map is [x, y] (the reference's); 1: [y, x] (this build's [H, W])
    int K, norm_bbox, merge;
    float osf, vs0, vs1, pc0, pc1;
    float coder_thr, test_thr, nms_thr;
    float coder_range[6], limit_range[6];
    int has_limit, pre_max, post_max;
    CenterTask task[CT_MAXTASKS];
    float* boxes;               // [B, ntasks, post_max, 9]
    float* scores;              // [B, ntasks, post_max]
    int* labels;
    int* counts;                // [B, ntasks]
    unsigned* keys;             // workspace [B, sumC, D0 * D1]: bits of sigmoid(logit)
};

// whole GPU: one thread per (sample, cell) writes the score keys of every class (a non-negative float's bits order like
// the float; NaN -> 0)
__global__ __launch_bounds__(256) void center_score_kernel(CenterParams p)
{
    const int64_t HW = (int64_t)p.D0 * p.D1;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)p.B * HW) return;
    const int64_t b = i / HW, cell = i % HW;
    const float* px = p.hout + i * p.CH;
    for (int t = 0; t < p.ntasks; ++t) {
        const CenterTask& tk = p.task[t];
        for (int c = 0; c < tk.ncls; ++c) {
            const float s = al3d_sigmoid(px[tk.heat_off + c]);
            p.keys[(b * p.sumC + tk.key_off + c) * HW + cell] = s == s ? __float_as_uint(s) : 0u;
        }
    }
}

// One workgroup per (sample, task).  LDS: 16 KB candidate keys, 32 KB corners, 4 KB areas, 1 KB live flags, 1 KB
// histogram, 2 KB pass list: 56 KB.
__global__ __launch_bounds__(CT_THREADS) void center_nms_kernel(CenterParams p)
{
    const int b = blockIdx.x / p.ntasks, t = blockIdx.x % p.ntasks;
    const CenterTask& tk = p.task[t];
    const int tid = threadIdx.x;
    const int HW = p.D0 * p.D1, K = p.K;

    __shared__ SelScratch<CT_THREADS> sel;
    __shared__ unsigned long long cand[CT_MAXCAND];     // sel_word(score bits, flat index)
    __shared__ float cx_s[CT_MAXK][4], cy_s[CT_MAXK][4];
    __shared__ float area_s[CT_MAXK];
    __shared__ unsigned char alive_s[CT_MAXK];
    __shared__ int pass_s[CT_MAXPOST];

    // ---- per class: the K best cells (ties: the smaller cell), by a four-pass radix select over the class's key plane
    for (int c = 0; c < tk.ncls; ++c) {
        const unsigned* __restrict__ kb = p.keys + ((int64_t)b * p.sumC + tk.key_off + c) * HW;
        unsigned T, need;
        blk_radix_threshold<CT_THREADS>(kb, HW, (unsigned)K, sel, T, need);
        blk_collect_topk<CT_THREADS>(kb, HW, T, need, (unsigned)(c * HW), cand + c * K, (unsigned)K, sel);
    }
    // ---- the K best of the ncls * K candidates: bitonic sort, (score descending, flat index ascending)
    const int total = tk.ncls * K;
    int N = 2;
    while (N < total) N <<= 1;
    for (int q = total + tid; q < N; q += CT_THREADS) cand[q] = 0ull;
    __syncthreads();
    blk_sort_desc_u64<CT_THREADS>(cand, N);
    // ---- gather + decode (coder :146-189), the coder's filters (:194-216) and, for the rotated NMS, the score filter of
    // get_task_detections (:814-824)
    float box[9];
    float score = 0.f;
    int label = 0;
    bool ok = false;
    if (tid < K) {
        const unsigned flat = sel_word_index(cand[tid]);
        label = (int)(flat / (unsigned)HW);
        const int cell = (int)(flat % (unsigned)HW);
        score = __uint_as_float(sel_word_bits(cand[tid]));
        const int d0 = cell / p.D1, d1 = cell % p.D1;
        float xs = (float)(p.swapped ? d1 : d0), ys = (float)(p.swapped ? d0 : d1);
        const float* px = p.hout + ((int64_t)b * HW + cell) * p.CH;
        if (tk.reg_off >= 0) { xs += px[tk.reg_off]; ys += px[tk.reg_off + 1]; }
        else { xs += 0.5f; ys += 0.5f; }
        box[0] = xs * p.osf * p.vs0 + p.pc0;
        box[1] = ys * p.osf * p.vs1 + p.pc1;
        box[2] = px[tk.hei_off];
#pragma unroll
        for (int k = 0; k < 3; ++k) box[3 + k] = p.norm_bbox ? expf(px[tk.dim_off + k]) : px[tk.dim_off + k];
        box[6] = atan2f(px[tk.rot_off], px[tk.rot_off + 1]);
        box[7] = tk.vel_off >= 0 ? px[tk.vel_off] : 0.f;
        box[8] = tk.vel_off >= 0 ? px[tk.vel_off + 1] : 0.f;
        ok = score > p.coder_thr &&
             box[0] >= p.coder_range[0] && box[1] >= p.coder_range[1] && box[2] >= p.coder_range[2] &&
             box[0] <= p.coder_range[3] && box[1] <= p.coder_range[4] && box[2] <= p.coder_range[5];
        if (tk.nms_kind == 0) ok = ok && score >= p.test_thr;
    }
    int n;
    int pos = blk_exclusive_scan<CT_THREADS>(ok ? 1 : 0, sel.wave, n);         // survivors stay in descending score order
    if (tk.nms_kind == 0 && n > p.pre_max) n = p.pre_max;
    ok = ok && pos < n;
    float x1 = 0.f, y1 = 0.f, x2 = 0.f, y2 = 0.f;
    if (ok) {
        alive_s[pos] = 1;
        if (tk.nms_kind == 0) {
            // BEV box (x, y, dim0 * s, dim1 * s, rot) -> corners x -+ w/2, y -+ l/2 turned about the centre (iou3d_kernel.cu:159-169)
            const float sc = tk.nms_scale[label];
            const float w = box[3] * sc, l = box[4] * sc;
            box_corners(box[0], box[1], w, l, box[6], cx_s[pos], cy_s[pos]);
            area_s[pos] = w * l;
            x1 = x2 = cx_s[pos][0]; y1 = y2 = cy_s[pos][0];
#pragma unroll
            for (int k = 1; k < 4; ++k) {
                x1 = fminf(x1, cx_s[pos][k]); x2 = fmaxf(x2, cx_s[pos][k]);
                y1 = fminf(y1, cy_s[pos][k]); y2 = fmaxf(y2, cy_s[pos][k]);
            }
        } else {
            cx_s[pos][0] = box[0];
            cy_s[pos][0] = box[1];
        }
    }
    __syncthreads();
    // ---- greedy suppression in score order: the best live candidate is kept and suppresses later ones; at most post_max kept
    const int post = p.post_max;
    int kept = 0, my_kpos = -1;
    bool live = ok;
    for (int i = 0; i < n && kept < post; ++i) {
        if (!alive_s[i]) continue;                  // workgroup-uniform: written before the last barrier
        if (ok && pos == i) my_kpos = kept;
        ++kept;
        if (kept == post) break;
        if (live && pos > i) {
            bool sup = false;
            if (tk.nms_kind == 1) {
                const float dx = cx_s[i][0] - box[0], dy = cy_s[i][0] - box[1];
                sup = dx * dx + dy * dy <= tk.radius;
            } else {
                float ax1 = cx_s[i][0], ax2 = ax1, ay1 = cy_s[i][0], ay2 = ay1;
#pragma unroll
                for (int k = 1; k < 4; ++k) {
                    ax1 = fminf(ax1, cx_s[i][k]); ax2 = fmaxf(ax2, cx_s[i][k]);
                    ay1 = fminf(ay1, cy_s[i][k]); ay2 = fmaxf(ay2, cy_s[i][k]);
                }
                // apart along an axis: no overlap, IoU = 0 <= nms_thr.  (NaN corners fall through to the clip.)
                const bool apart = ax2 < x1 || x2 < ax1 || ay2 < y1 || y2 < ay1;
                if (!apart) {
                    const float inter = quad_intersection_area(cx_s[i], cy_s[i], cx_s[pos], cy_s[pos]);
                    const float iou = inter / fmaxf(area_s[i] + area_s[pos] - inter, 1e-8f);
                    sup = iou > p.nms_thr;
                }
            }
            if (sup) { alive_s[pos] = 0; live = false; }
        }
        __syncthreads();
    }
    // ---- write: kept order; the rotated path applies post_center_limit_range after the NMS (:860-867); merge (:738-757)
    const bool mine = my_kpos >= 0;
    bool pass = mine;
    if (mine && tk.nms_kind == 0 && p.has_limit)
        pass = box[0] >= p.limit_range[0] && box[1] >= p.limit_range[1] && box[2] >= p.limit_range[2] &&
               box[0] <= p.limit_range[3] && box[1] <= p.limit_range[4] && box[2] <= p.limit_range[5];
    if (mine) pass_s[my_kpos] = pass ? 1 : 0;
    __syncthreads();
    if (mine && pass) {
        int dst = 0;
        for (int q = 0; q < my_kpos; ++q) dst += pass_s[q];
        const int64_t o = ((int64_t)b * p.ntasks + t) * p.post_max + dst;
        if (p.merge) box[2] = box[2] - box[5] * 0.5f;
#pragma unroll
        for (int k = 0; k < 9; ++k) p.boxes[o * 9 + k] = box[k];
        p.scores[o] = score;
        p.labels[o] = label + (p.merge ? tk.label_off : 0);
    }
    if (tid == 0) {
        int cnt = 0;
        for (int q = 0; q < kept; ++q) cnt += pass_s[q];
        p.counts[b * p.ntasks + t] = cnt;
    }
}

extern "C" int64_t al3d_center_decode_nms_workspace_bytes(int B, int D0, int D1, int sum_classes)
{
    return al3d_align((int64_t)(B > 0 ? B : 1) * D0 * D1 * (sum_classes > 0 ? sum_classes : 1) * 4, 256);
}

extern "C" int al3d_center_decode_nms_f32(const float* hout, int B, int D0, int D1, int CH, int swapped, int ntasks,
                                          const int* task_ncls, const int* chan_off, int max_num, int norm_bbox,
                                          const float* geom5, float coder_score_thr, const float* coder_range6,
                                          const int* nms_kind, const float* nms_scale, const float* min_radius,
                                          float test_score_thr, float nms_thr, int pre_max, int post_max,
                                          const float* limit_range6, int merge, float* boxes, float* scores, int* labels,
                                          int* counts, void* workspace, void* stream)
{
    AL3D_REQUIRE(ntasks >= 1 && ntasks <= CT_MAXTASKS, "al3d_center_decode_nms_f32: ntasks must be in [1,%d]", CT_MAXTASKS);
    AL3D_REQUIRE(B >= 0 && D0 > 0 && D1 > 0 && CH > 0, "al3d_center_decode_nms_f32: bad map sizes");
    AL3D_REQUIRE(task_ncls && chan_off && geom5 && coder_range6 && nms_kind && nms_scale && min_radius,
                 "al3d_center_decode_nms_f32: null pointer");
    AL3D_REQUIRE(max_num >= 1 && max_num <= CT_MAXK, "al3d_center_decode_nms_f32: max_num must be in [1,%d]", CT_MAXK);
    AL3D_REQUIRE((int64_t)D0 * D1 >= max_num, "al3d_center_decode_nms_f32: max_num %d exceeds the %d x %d cells of the map", max_num,
                 D0, D1);
    AL3D_REQUIRE(post_max >= 1 && post_max <= CT_MAXPOST, "al3d_center_decode_nms_f32: post_max must be in [1,%d]", CT_MAXPOST);
    AL3D_REQUIRE(pre_max >= 1, "al3d_center_decode_nms_f32: pre_max must be positive");
    CenterParams p;
    p.hout = hout; p.B = B; p.D0 = D0; p.D1 = D1; p.CH = CH; p.ntasks = ntasks; p.swapped = swapped ? 1 : 0;
    p.K = max_num; p.norm_bbox = norm_bbox ? 1 : 0; p.merge = merge ? 1 : 0;
    p.osf = geom5[0]; p.vs0 = geom5[1]; p.vs1 = geom5[2]; p.pc0 = geom5[3]; p.pc1 = geom5[4];
    p.coder_thr = coder_score_thr; p.test_thr = test_score_thr; p.nms_thr = nms_thr;
    p.has_limit = limit_range6 != nullptr; p.pre_max = pre_max; p.post_max = post_max;
    for (int k = 0; k < 6; ++k) { p.coder_range[k] = coder_range6[k]; p.limit_range[k] = limit_range6 ? limit_range6[k] : 0.f; }
    int sumC = 0;
    for (int t = 0; t < ntasks; ++t) {
        CenterTask& tk = p.task[t];
        tk.ncls = task_ncls[t];
        AL3D_REQUIRE(tk.ncls >= 1 && tk.ncls <= CT_MAXCLS && tk.ncls * max_num <= CT_MAXCAND,
                     "al3d_center_decode_nms_f32: task %d: classes must be in [1,%d] and classes x max_num <= %d", t, CT_MAXCLS, CT_MAXCAND);
        const int* o = chan_off + 6 * t;             // heatmap, reg, height, dim, rot, vel
        tk.heat_off = o[0]; tk.reg_off = o[1]; tk.hei_off = o[2]; tk.dim_off = o[3]; tk.rot_off = o[4]; tk.vel_off = o[5];
        AL3D_REQUIRE(tk.heat_off >= 0 && tk.heat_off + tk.ncls <= CH && tk.hei_off >= 0 && tk.hei_off < CH && tk.dim_off >= 0 &&
                     tk.dim_off + 3 <= CH && tk.rot_off >= 0 && tk.rot_off + 2 <= CH && tk.reg_off + 2 <= CH && tk.vel_off + 2 <= CH &&
                     tk.reg_off >= -1 && tk.vel_off >= -1,
                     "al3d_center_decode_nms_f32: task %d channel window exceeds CH", t);
        AL3D_REQUIRE(nms_kind[t] == 0 || nms_kind[t] == 1, "al3d_center_decode_nms_f32: nms kind must be 0 (rotate) or 1 (circle)");
        tk.nms_kind = nms_kind[t]; tk.radius = min_radius[t];
        for (int c = 0; c < CT_MAXCLS; ++c) tk.nms_scale[c] = c < tk.ncls ? nms_scale[t * CT_MAXCLS + c] : 1.f;
        tk.key_off = sumC; tk.label_off = sumC;
        sumC += tk.ncls;
    }
    p.sumC = sumC;
    AL3D_REQUIRE((int64_t)D0 * D1 * CT_MAXCLS < (1ll << 31), "al3d_center_decode_nms_f32: map too large");
    if (B == 0) return AL3D_OK;
    AL3D_REQUIRE(hout && boxes && scores && labels && counts && workspace, "al3d_center_decode_nms_f32: null pointer");
    p.boxes = boxes; p.scores = scores; p.labels = labels; p.counts = counts; p.keys = (unsigned*)workspace;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(center_score_kernel, dim3((unsigned)al3d_cdiv((int64_t)B * D0 * D1, 256)), dim3(256), 0, s, p);
    hipLaunchKernelGGL(center_nms_kernel, dim3((unsigned)(B * ntasks)), dim3(CT_THREADS), 0, s, p);
    AL3D_CHECK_LAUNCH("al3d_center_decode_nms_f32");
    return AL3D_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// The last convolutions of the separate heads (centerpoint.py:76-86): 3x3, stride 1, padding 1, 64 -> 1..8 channels,
// bias; G of them in one launch.  x [B, H, W, G * 64]: group g reads channels g*64 .. g*64+63 and writes cout[g]
// channels at coff[g] of out [B, H, W, ldc].  One thread per output pixel, the group's weights ([cout][9][64], tap =
// ky * 3 + kx) staged in LDS (<= 18 KB) and read as broadcasts; f32 FMAs, taps in order, channels ascending.
#define GC_THREADS 256
#define GC_MAXG 64

struct GroupTab { int cout[GC_MAXG], coff[GC_MAXG], wrow[GC_MAXG]; };

template <int N>
__device__ __forceinline__ void gconv_body(const float* __restrict__ x, const float* __restrict__ w_s, const float* __restrict__ bias,
                                           float* __restrict__ out, int64_t pix, int H, int W, int C, int g, int ldc, int coff, int cout)
{
    const int xw = (int)(pix % W), yh = (int)((pix / W) % H);
    float acc[N];
#pragma unroll
    for (int o = 0; o < N; ++o) acc[o] = o < cout ? bias[o] : 0.f;
    for (int tap = 0; tap < 9; ++tap) {
        const int iy = yh + tap / 3 - 1, ix = xw + tap % 3 - 1;
        if (iy < 0 || iy >= H || ix < 0 || ix >= W) continue;
        const float4* __restrict__ px = reinterpret_cast<const float4*>(x + (pix + (int64_t)(tap / 3 - 1) * W + (tap % 3 - 1)) * C + g * 64);
#pragma unroll 4
        for (int c4 = 0; c4 < 16; ++c4) {
            const float4 v = px[c4];
#pragma unroll
            for (int o = 0; o < N; ++o) {
                const float4 w = *reinterpret_cast<const float4*>(w_s + (o * 9 + tap) * 64 + c4 * 4);
                acc[o] = fmaf(v.x, w.x, acc[o]);
                acc[o] = fmaf(v.y, w.y, acc[o]);
                acc[o] = fmaf(v.z, w.z, acc[o]);
                acc[o] = fmaf(v.w, w.w, acc[o]);
            }
        }
    }
#pragma unroll
    for (int o = 0; o < N; ++o)
        if (o < cout) out[pix * ldc + coff + o] = acc[o];
}

__global__ __launch_bounds__(GC_THREADS) void gconv3x3_kernel(const float* __restrict__ x, const float* __restrict__ wts,
                                                              const float* __restrict__ bias, float* __restrict__ out, int64_t npix,
                                                              int H, int W, int G, int ldc, GroupTab tab)
{
    __shared__ __attribute__((aligned(16))) float w_s[8 * 9 * 64];
    const int g = blockIdx.y, cout = tab.cout[g];
    const int n = cout <= 4 ? cout : 8;
    for (int e = threadIdx.x; e < n * 576; e += GC_THREADS) w_s[e] = e < cout * 576 ? wts[(int64_t)tab.wrow[g] * 576 + e] : 0.f;
    __syncthreads();
    const int64_t pix = (int64_t)blockIdx.x * GC_THREADS + threadIdx.x;
    if (pix >= npix) return;
    const float* bg = bias + tab.wrow[g];
    const int C = G * 64, coff = tab.coff[g];
    switch (n) {
    case 1: gconv_body<1>(x, w_s, bg, out, pix, H, W, C, g, ldc, coff, cout); break;
    case 2: gconv_body<2>(x, w_s, bg, out, pix, H, W, C, g, ldc, coff, cout); break;
    case 3: gconv_body<3>(x, w_s, bg, out, pix, H, W, C, g, ldc, coff, cout); break;
    case 4: gconv_body<4>(x, w_s, bg, out, pix, H, W, C, g, ldc, coff, cout); break;
    default: gconv_body<8>(x, w_s, bg, out, pix, H, W, C, g, ldc, coff, cout); break;
    }
}

extern "C" int al3d_conv3x3_grouped_nhwc_f32(const float* x, const float* w, const float* bias, float* out, int B, int H, int W,
                                             int G, const int* cout, const int* coff, int ldc, void* stream)
{
    AL3D_REQUIRE(B >= 0 && H > 0 && W > 0 && G >= 1 && G <= GC_MAXG && ldc >= 1, "al3d_conv3x3_grouped_nhwc_f32: bad sizes (1 <= groups <= %d)",
                 GC_MAXG);
    AL3D_REQUIRE(cout && coff, "al3d_conv3x3_grouped_nhwc_f32: null pointer");
    AL3D_REQUIRE((int64_t)B * H * W * G * 64 < (1ll << 40) && (int64_t)B * H * W < (1ll << 31) * GC_THREADS,
                 "al3d_conv3x3_grouped_nhwc_f32: map too large");
    GroupTab tab;
    int rows = 0;
    for (int g = 0; g < G; ++g) {
        AL3D_REQUIRE(cout[g] >= 1 && cout[g] <= 8, "al3d_conv3x3_grouped_nhwc_f32: group %d: 1 <= cout <= 8", g);
        AL3D_REQUIRE(coff[g] >= 0 && coff[g] + cout[g] <= ldc, "al3d_conv3x3_grouped_nhwc_f32: group %d writes outside the %d output channels",
                     g, ldc);
        tab.cout[g] = cout[g]; tab.coff[g] = coff[g]; tab.wrow[g] = rows;
        rows += cout[g];
    }
    if (B == 0) return AL3D_OK;
    AL3D_REQUIRE(x && w && bias && out, "al3d_conv3x3_grouped_nhwc_f32: null pointer");
    const int64_t npix = (int64_t)B * H * W;
    hipLaunchKernelGGL(gconv3x3_kernel, dim3((unsigned)al3d_cdiv(npix, GC_THREADS), (unsigned)G), dim3(GC_THREADS), 0, (hipStream_t)stream,
                       x, w, bias, out, npix, H, W, G, ldc, tab);
    AL3D_CHECK_LAUNCH("al3d_conv3x3_grouped_nhwc_f32");
    return AL3D_OK;
}
