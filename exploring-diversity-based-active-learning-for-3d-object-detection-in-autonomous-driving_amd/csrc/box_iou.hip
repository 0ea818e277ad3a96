// Box geometry as ops of its own (include/al3d.h "rotated box IoU and NMS"): the N x M IoU matrix, the per-frame best IoU of
// every detection against reference boxes on the raw NMS buffers, and a stand-alone greedy NMS.  They replace det3d's
// iou3d_nms extension (det3d/ops/iou3d_nms/iou3d_nms_utils.py:13-107, src/iou3d_nms_kernel.cu), mmdet3d's iou3d extension
// (bevfusion/mmdet3d/ops/iou3d/iou3d_utils.py:6-68, src/iou3d_kernel.cu) and the numba.cuda kernel of the in-tree KITTI
// evaluation (det3d/datasets/utils/kitti_object_eval_python/rotate_iou.py:250-341).  The rectangle intersection is
// al3d_rbox.h's, unchanged: the reference's clipping code is not ported.
//
// Shape of all three: a box becomes a record once per workgroup -- its four corners (one sinf / cosf), footprint area,
// centre, bounding-circle radius, height interval, volume, a "finite" flag -- in LDS, struct-of-arrays so that the 64 lanes
// of a wave read 64 consecutive words.  A wave then takes one row box (a broadcast read) against 64 column boxes, ONE PAIR
// PER LANE: the matrix stores 64 consecutive floats, the reduction takes a wave-wide maximum, the NMS a wave-wide ballot
// (64 lanes = the 64 bits of a mask word).  Pairs whose bounding circles are apart skip the clip: most pairs of a frame.
// Every result is a function of its pair alone, the maximum and the ballot do not depend on an order, and the greedy walk
// is sequential: all outputs are bit-identical from run to run and for every launch shape.  f32 on the VALU, no contraction.
#include "al3d_common.h"
#include "al3d_rbox.h"
#include "al3d_select.h"

#define BOX_TILE 64              // column boxes of a tile = lanes of a wave
#define BOX_ROWS_MAX 128         // row boxes a workgroup holds at a time
#define NMS_MAX 4096             // AL3D_NMS_MAX_CANDIDATES
#define NMS_WORDS (NMS_MAX / 64)

template <int CAP>
struct BoxTile {
    float cx[4][CAP], cy[4][CAP];
    float area[CAP], mx[CAP], my[CAP], rad[CAP], hx[CAP], hy[CAP], zlo[CAP], zhi[CAP], vol[CAP];
    int ok[CAP];
};

struct BoxFormat { int dim, rot, layout, convention, height; };

// one row of boxes -> slot s of the tile.  A row with a NaN or an inf among its seven numbers, or with a footprint size that
// is not positive, is not a box: ok = 0, and every pair it takes part in gives 0.
template <int CAP>
__device__ __forceinline__ void box_record(const float* __restrict__ row, const BoxFormat f, BoxTile<CAP>& t, int s)
{
    float x, y, z = 0.f, s0, s1, h = 0.f, r;
    if (f.layout == AL3D_BOX_ROWS_XYXYR) {
        const float x1 = row[0], y1 = row[1], x2 = row[2], y2 = row[3];
        x = 0.5f * (x1 + x2); y = 0.5f * (y1 + y2); s0 = x2 - x1; s1 = y2 - y1; r = row[4];
    } else {
        x = row[0]; y = row[1]; z = row[2]; s0 = row[3]; s1 = row[4]; h = row[5]; r = row[f.rot];
    }
    const bool ok = isfinite(x) && isfinite(y) && isfinite(z) && isfinite(s0) && isfinite(s1) && isfinite(h) && isfinite(r) &&
                    s0 > 0.f && s1 > 0.f;
    if (!ok) x = y = z = s0 = s1 = h = r = 0.f;
    float cx[4], cy[4];
    // HEADING turns the other way: cos is even and sinf odd, so this is centre + [[cos,-sin],[sin,cos]] (+-s0/2, +-s1/2)
    box_corners(x, y, s0, s1, f.convention == AL3D_BOX_HEADING ? -r : r, cx, cy);
#pragma unroll
    for (int k = 0; k < 4; ++k) { t.cx[k][s] = cx[k]; t.cy[k][s] = cy[k]; }
    t.area[s] = quad_area(cx, cy);
    t.mx[s] = x; t.my[s] = y;
    t.hx[s] = 0.5f * s0; t.hy[s] = 0.5f * s1;
    t.rad[s] = 0.5f * sqrtf(s0 * s0 + s1 * s1);
    if (f.height == AL3D_IOU_H_TOP) { t.zlo[s] = z - h; t.zhi[s] = z; }
    else { t.zlo[s] = z - 0.5f * h; t.zhi[s] = z + 0.5f * h; }
    t.vol[s] = s0 * s1 * h;
    t.ok[s] = ok ? 1 : 0;
}

// the footprints' intersection area of row box i and column box j.  The circle test leaves 1e-4 of slack, far more than the
// rounding of the radii and of the distance: a pair it rejects is apart by a real gap and its exact intersection is empty.
template <int CA, int CB>
__device__ __forceinline__ float pair_inter(const BoxTile<CA>& A, int i, const BoxTile<CB>& B, int j, int reject)
{
    const float dx = A.mx[i] - B.mx[j], dy = A.my[i] - B.my[j], rr = A.rad[i] + B.rad[j];
    if (reject && dx * dx + dy * dy > rr * rr * 1.0001f) return 0.f;
    float ax[4], ay[4], bx[4], by[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) { ax[k] = A.cx[k][i]; ay[k] = A.cy[k][i]; bx[k] = B.cx[k][j]; by[k] = B.cy[k][j]; }
    return quad_intersection_area(ax, ay, bx, by);
}

template <int CA, int CB>
__device__ __forceinline__ float pair_value(const BoxTile<CA>& A, int i, const BoxTile<CB>& B, int j, int metric, int height,
                                            int reject)
{
    if (!(A.ok[i] && B.ok[j])) return 0.f;
    float inter = pair_inter(A, i, B, j, reject);
    float sa = A.area[i], sb = B.area[j], eps = 1e-8f;
    if (height != AL3D_IOU_H_NONE) {
        inter *= fmaxf(fminf(A.zhi[i], B.zhi[j]) - fmaxf(A.zlo[i], B.zlo[j]), 0.f);
        sa = A.vol[i]; sb = B.vol[j]; eps = 1e-6f;
    }
    float v = inter;
    if (metric == AL3D_IOU_IOU) v = inter / fmaxf(sa + sb - inter, eps);
    else if (metric == AL3D_IOU_OVER_A) v = inter / fmaxf(sa, eps);
    else if (metric == AL3D_IOU_OVER_B) v = inter / fmaxf(sb, eps);
    return v == v ? v : 0.f;                            // sizes that overflow: 0, not NaN
}

// iou_normal of iou3d_nms_kernel.cu:314-325: the axis-aligned boxes x +- dx/2, y +- dy/2, the angle ignored
template <int CA, int CB>
__device__ __forceinline__ float pair_normal(const BoxTile<CA>& A, int i, const BoxTile<CB>& B, int j)
{
    if (!(A.ok[i] && B.ok[j])) return 0.f;
    const float left = fmaxf(A.mx[i] - A.hx[i], B.mx[j] - B.hx[j]), right = fminf(A.mx[i] + A.hx[i], B.mx[j] + B.hx[j]);
    const float top = fmaxf(A.my[i] - A.hy[i], B.my[j] - B.hy[j]), bottom = fminf(A.my[i] + A.hy[i], B.my[j] + B.hy[j]);
    const float inter = fmaxf(right - left, 0.f) * fmaxf(bottom - top, 0.f);
    const float sa = (2.f * A.hx[i]) * (2.f * A.hy[i]), sb = (2.f * B.hx[j]) * (2.f * B.hy[j]);
    const float v = inter / fmaxf(sa + sb - inter, 1e-8f);
    return v == v ? v : 0.f;
}

// ---------------------------------------------------------------- (a) the matrix
// workgroup = a tile of `ta` rows x 64 columns; wave w takes rows w, w + waves, ...
__global__ __launch_bounds__(256) void box_iou_matrix_kernel(const float* __restrict__ a, int N, BoxFormat fa,
                                                             const float* __restrict__ b, int M, BoxFormat fb, int metric,
                                                             int reject, int ta, int tiles_m, float* __restrict__ out)
{
    __shared__ BoxTile<BOX_ROWS_MAX> sA;
    __shared__ BoxTile<BOX_TILE> sB;
    const int tn = blockIdx.x / tiles_m, tm = blockIdx.x - tn * tiles_m;
    const int n0 = tn * ta, m0 = tm * BOX_TILE;
    for (int s = threadIdx.x; s < ta + BOX_TILE; s += blockDim.x) {
        if (s < ta) { if (n0 + s < N) box_record(a + (int64_t)(n0 + s) * fa.dim, fa, sA, s); }
        else if (m0 + s - ta < M) box_record(b + (int64_t)(m0 + s - ta) * fb.dim, fb, sB, s - ta);
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
    if (m0 + lane >= M) return;
    for (int i = wave; i < ta && n0 + i < N; i += waves)
        out[(int64_t)(n0 + i) * M + m0 + lane] = pair_value(sA, i, sB, lane, metric, fa.height, reject);
}

static int box_format_check(const char* who, int dim, int rot, int layout, int convention, int height)
{
    AL3D_REQUIRE(layout == AL3D_BOX_ROWS_XYZ || layout == AL3D_BOX_ROWS_XYXYR, "%s: bad layout", who);
    AL3D_REQUIRE(convention == AL3D_BOX_DET3D || convention == AL3D_BOX_HEADING, "%s: bad convention", who);
    AL3D_REQUIRE(height == AL3D_IOU_H_NONE || height == AL3D_IOU_H_CENTRE || height == AL3D_IOU_H_TOP, "%s: bad height rule", who);
    if (layout == AL3D_BOX_ROWS_XYXYR) {
        AL3D_REQUIRE(dim >= 5, "%s: [x1, y1, x2, y2, r] rows need box_dim >= 5", who);
        AL3D_REQUIRE(height == AL3D_IOU_H_NONE, "%s: [x1, y1, x2, y2, r] rows have no height", who);
    } else {
        AL3D_REQUIRE(dim >= 7, "%s: box_dim must be >= 7", who);
        AL3D_REQUIRE(rot >= 6 && rot < dim, "%s: rot_col must lie in [6, box_dim)", who);
    }
    return AL3D_OK;
}

static int metric_check(const char* who, int metric)
{
    AL3D_REQUIRE(metric == AL3D_IOU_OVERLAP || metric == AL3D_IOU_IOU || metric == AL3D_IOU_OVER_A || metric == AL3D_IOU_OVER_B,
                 "%s: bad metric", who);
    return AL3D_OK;
}

extern "C" int al3d_box_iou_matrix_launch_f32(const float* a, int64_t N, int a_dim, int a_rot, const float* b, int64_t M,
                                              int b_dim, int b_rot, int layout, int convention, int metric, int height,
                                              float* out, int tile_rows, int threads, int reject, void* stream)
{
    const char* who = "al3d_box_iou_matrix_f32";
    AL3D_REQUIRE(N >= 0 && M >= 0 && N < (1LL << 31) && M < (1LL << 31), "%s: bad sizes", who);
    if (box_format_check(who, a_dim, a_rot, layout, convention, height) || box_format_check(who, b_dim, b_rot, layout, convention, height) ||
        metric_check(who, metric))
        return AL3D_EINVAL;
    AL3D_REQUIRE(tile_rows >= 1 && tile_rows <= BOX_ROWS_MAX && (threads == 64 || threads == 128 || threads == 256),
                 "%s: tile_rows in [1, %d] and 64, 128 or 256 threads", who, BOX_ROWS_MAX);
    if (N == 0 || M == 0) return AL3D_OK;
    AL3D_REQUIRE(a && b && out, "%s: null pointer", who);
    const int64_t tiles_m = al3d_cdiv(M, BOX_TILE), tiles = al3d_cdiv(N, tile_rows) * tiles_m;
    AL3D_REQUIRE(tiles < (1LL << 31), "%s: too many tiles", who);
    const BoxFormat fa = {a_dim, a_rot, layout, convention, height}, fb = {b_dim, b_rot, layout, convention, height};
    hipLaunchKernelGGL(box_iou_matrix_kernel, dim3((unsigned)tiles), dim3(threads), 0, (hipStream_t)stream, a, (int)N, fa, b,
                       (int)M, fb, metric, reject ? 1 : 0, tile_rows, (int)tiles_m, out);
    AL3D_CHECK_LAUNCH("box_iou_matrix_kernel");
    return AL3D_OK;
}

extern "C" int al3d_box_iou_matrix_f32(const float* a, int64_t N, int a_dim, int a_rot, const float* b, int64_t M, int b_dim,
                                       int b_rot, int layout, int convention, int metric, int height, float* out, void* stream)
{
    return al3d_box_iou_matrix_launch_f32(a, N, a_dim, a_rot, b, M, b_dim, b_rot, layout, convention, metric, height, out,
                                          AL3D_BOX_IOU_TILE_ROWS, 256, 1, stream);
}

// ---------------------------------------------------------------- (b) best IoU per detection
// workgroup = one (frame, task).  Its slots go into LDS `chunk` at a time; the frame's reference rows pass by in tiles of
// `rtile` <= 64, ascending.  A wave takes one slot against the tile, one pair per lane, and reduces (value, row) to the
// largest value, the lowest row among equal ones; lane 0 keeps the slot's running best, replaced only by a strictly larger
// value, so an earlier tile keeps a tie.
__global__ __launch_bounds__(256) void box_iou_best_kernel(const float* __restrict__ boxes, const int* __restrict__ labels,
                                                           const int* __restrict__ counts, int post, BoxFormat fp,
                                                           const float* __restrict__ ref_boxes,
                                                           const int* __restrict__ ref_labels, const int* __restrict__ ref_off,
                                                           int R, BoxFormat fr, int metric, int same_class, int reject, int chunk,
                                                           int rtile, float* __restrict__ best_iou, int* __restrict__ best_ref,
                                                           int* __restrict__ status)
{
    __shared__ BoxTile<BOX_ROWS_MAX> sA;
    __shared__ BoxTile<BOX_TILE> sB;
    __shared__ int s_alabel[BOX_ROWS_MAX], s_blabel[BOX_TILE], s_ref[BOX_ROWS_MAX];
    __shared__ float s_val[BOX_ROWS_MAX];
    const int t = blockIdx.x, b = blockIdx.y, nt = gridDim.x;      // grid = (nt, B)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
    const int64_t base = ((int64_t)b * nt + t) * post;
    const int cnt = min(max(counts[b * nt + t], 0), post);
    int r0 = ref_off[b], r1 = ref_off[b + 1];
    if (r0 < 0 || r1 < r0 || r1 > R) {
        if (threadIdx.x == 0) atomicOr(status, AL3D_IOU_BAD_OFFSETS);
        r0 = r1 = 0;
    }
    for (int c0 = 0; c0 < post; c0 += chunk) {
        const int nc = min(chunk, cnt - c0);               // valid slots of this chunk (may be <= 0)
        for (int s = threadIdx.x; s < nc; s += blockDim.x) {
            box_record(boxes + (base + c0 + s) * fp.dim, fp, sA, s);
            s_alabel[s] = labels[base + c0 + s];
            s_val[s] = -1.f;
            s_ref[s] = -1;
        }
        __syncthreads();
        for (int t0 = r0; t0 < r1 && nc > 0; t0 += rtile) {
            const int nr = min(rtile, r1 - t0);
            for (int s = threadIdx.x; s < nr; s += blockDim.x) {
                box_record(ref_boxes + (int64_t)(t0 + s) * fr.dim, fr, sB, s);
                s_blabel[s] = ref_labels[t0 + s];
            }
            __syncthreads();
            for (int i = wave; i < nc; i += waves) {
                float v = -1.f;
                int row = 0x7fffffff;
                if (lane < nr && (!same_class || s_blabel[lane] == s_alabel[i])) {
                    v = pair_value(sA, i, sB, lane, metric, fp.height, reject);
                    row = t0 + lane;
                }
                for (int off = 32; off > 0; off >>= 1) {
                    const float ov = __shfl_xor(v, off);
                    const int orow = __shfl_xor(row, off);
                    if (ov > v || (ov == v && orow < row)) { v = ov; row = orow; }
                }
                if (lane == 0 && row != 0x7fffffff && v > s_val[i]) { s_val[i] = v; s_ref[i] = row; }
            }
            __syncthreads();
        }
        for (int s = threadIdx.x; s < min(chunk, post - c0); s += blockDim.x) {
            const bool hit = s < nc && s_ref[s] >= 0;
            best_iou[base + c0 + s] = hit ? s_val[s] : 0.f;
            best_ref[base + c0 + s] = hit ? s_ref[s] : -1;
        }
        __syncthreads();
    }
}

extern "C" int al3d_box_iou_best_launch_f32(const float* boxes, const int* labels, const int* counts, int B, int nt, int post,
                                            int box_dim, int rot_col, const float* ref_boxes, const int* ref_labels,
                                            const int* ref_off, int R, int ref_dim, int ref_rot, int convention, int metric,
                                            int height, int same_class, float* best_iou, int* best_ref, int* status,
                                            int chunk, int ref_tile, int threads, int reject, void* stream)
{
    const char* who = "al3d_box_iou_best_f32";
    AL3D_REQUIRE(B >= 0 && nt >= 1 && post >= 1 && R >= 0, "%s: bad sizes", who);
    AL3D_REQUIRE((int64_t)B * nt * post < (1LL << 31) / (box_dim > 0 ? box_dim : 1) && B < 65536, "%s: batch too large", who);
    if (box_format_check(who, box_dim, rot_col, AL3D_BOX_ROWS_XYZ, convention, height) ||
        box_format_check(who, ref_dim, ref_rot, AL3D_BOX_ROWS_XYZ, convention, height) || metric_check(who, metric))
        return AL3D_EINVAL;
    AL3D_REQUIRE(chunk >= 1 && chunk <= BOX_ROWS_MAX && ref_tile >= 1 && ref_tile <= BOX_TILE &&
                 (threads == 64 || threads == 128 || threads == 256),
                 "%s: chunk in [1, %d], ref_tile in [1, %d] and 64, 128 or 256 threads", who, BOX_ROWS_MAX, BOX_TILE);
    AL3D_REQUIRE(status, "%s: null pointer", who);
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(status, 0, sizeof(int), st) != hipSuccess) return al3d_fail(AL3D_ELAUNCH, "%s: memset", who);
    if (B == 0) return AL3D_OK;
    AL3D_REQUIRE(boxes && labels && counts && ref_off && best_iou && best_ref, "%s: null pointer", who);
    AL3D_REQUIRE(R == 0 || (ref_boxes && ref_labels), "%s: null pointer", who);
    const BoxFormat fp = {box_dim, rot_col, AL3D_BOX_ROWS_XYZ, convention, height},
                    fr = {ref_dim, ref_rot, AL3D_BOX_ROWS_XYZ, convention, height};
    hipLaunchKernelGGL(box_iou_best_kernel, dim3((unsigned)nt, (unsigned)B), dim3(threads), 0, st, boxes, labels, counts, post,
                       fp, ref_boxes, ref_labels, ref_off, R, fr, metric, same_class ? 1 : 0, reject ? 1 : 0, chunk, ref_tile,
                       best_iou, best_ref, status);
    AL3D_CHECK_LAUNCH("box_iou_best_kernel");
    return AL3D_OK;
}

extern "C" int al3d_box_iou_best_f32(const float* boxes, const int* labels, const int* counts, int B, int nt, int post,
                                     int box_dim, int rot_col, const float* ref_boxes, const int* ref_labels, const int* ref_off,
                                     int R, int ref_dim, int ref_rot, int convention, int metric, int height, int same_class,
                                     float* best_iou, int* best_ref, int* status, void* stream)
{
    return al3d_box_iou_best_launch_f32(boxes, labels, counts, B, nt, post, box_dim, rot_col, ref_boxes, ref_labels, ref_off, R,
                                        ref_dim, ref_rot, convention, metric, height, same_class, best_iou, best_ref, status,
                                        BOX_ROWS_MAX, BOX_TILE, 256, 1, stream);
}

// ---------------------------------------------------------------- (c) stand-alone NMS
// 1. the K best scores in descending order (al3d_sort_key.h: NaN last, equal scores by ascending index): one workgroup
template <int THREADS>
__global__ __launch_bounds__(THREADS) void nms_order_kernel(const float* __restrict__ scores, int N, int K,
                                                            unsigned* __restrict__ keys, int* __restrict__ order)
{
    __shared__ unsigned long long s_w[NMS_MAX];
    __shared__ SelScratch<THREADS> s;
    int n = N;                                              // words in s_w
    if (N <= NMS_MAX) {
        for (int i = threadIdx.x; i < N; i += THREADS) s_w[i] = al3d_sort_key(scores[i], (unsigned)i);
    } else {
        for (int i = threadIdx.x; i < N; i += THREADS) keys[i] = sel_word_bits(al3d_sort_key(scores[i], (unsigned)i));
        __syncthreads();
        unsigned T, need;
        blk_radix_threshold<THREADS>(keys, N, (unsigned)K, s, T, need);
        blk_collect_topk<THREADS>(keys, N, T, need, 0u, s_w, NMS_MAX, s);
        n = K;
    }
    int np2 = 1;
    while (np2 < n) np2 <<= 1;
    for (int i = n + threadIdx.x; i < np2; i += THREADS) s_w[i] = 0ull;      // below every real word
    __syncthreads();
    blk_sort_desc_u64<THREADS, int>(s_w, np2);
    for (int i = threadIdx.x; i < K; i += THREADS) order[i] = (int)sel_word_index(s_w[i]);
}

// 2. the suppression bits: workgroup = (row tile, column tile) of 64 x 64 candidates in rank order, column tile >= row tile.
//    A wave takes a row against the 64 columns; its ballot is the mask word (iou3d_nms_kernel.cu:282-311's word, built by
//    64 lanes instead of one thread's loop).
__global__ __launch_bounds__(256) void nms_mask_kernel(const float* __restrict__ boxes, BoxFormat f, const int* __restrict__ order,
                                                       int K, int mode, float thresh, int reject,
                                                       unsigned long long* __restrict__ mask)
{
    __shared__ BoxTile<BOX_TILE> sA, sB;
    const int rt = blockIdx.y, ct = blockIdx.x;
    if (ct < rt) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
    for (int s = threadIdx.x; s < 2 * BOX_TILE; s += blockDim.x) {
        const int k = (s < BOX_TILE ? rt : ct) * BOX_TILE + (s & 63);
        if (k < K) {
            if (s < BOX_TILE) box_record(boxes + (int64_t)order[k] * f.dim, f, sA, s);
            else box_record(boxes + (int64_t)order[k] * f.dim, f, sB, s - BOX_TILE);
        }
    }
    __syncthreads();
    const int col = ct * BOX_TILE + lane;
    for (int i = wave; i < BOX_TILE; i += waves) {
        const int row = rt * BOX_TILE + i;
        if (row >= K) break;
        bool hit = false;
        if (col < K && col > row) {
            const float v = mode == AL3D_NMS_NORMAL ? pair_normal(sA, i, sB, lane)
                                                    : pair_value(sA, i, sB, lane, AL3D_IOU_IOU, AL3D_IOU_H_NONE, reject);
            hit = v > thresh;
        }
        const unsigned long long word = __ballot(hit);
        if (lane == 0) mask[(int64_t)row * NMS_WORDS + ct] = word;
    }
}

// 3. the greedy walk: one wave, lane w holds word w of the removed set.  A step needs the mask row of a kept candidate; the
//    rows of the next NMS_AHEAD candidates are loaded before they are known to be kept, so a step does not wait for HBM
#define NMS_AHEAD 8
__global__ __launch_bounds__(64) void nms_walk_kernel(const unsigned long long* __restrict__ mask, const int* __restrict__ order,
                                                      int K, int post_max, int* __restrict__ keep, int* __restrict__ count)
{
    const int lane = threadIdx.x, words = (K + 63) >> 6;
    const bool mine = lane < words;
    unsigned long long removed = 0ull, ahead[NMS_AHEAD];
#pragma unroll
    for (int d = 0; d < NMS_AHEAD; ++d) ahead[d] = (mine && d < K) ? mask[(int64_t)d * NMS_WORDS + lane] : 0ull;
    int n = 0;
    bool full = false;
    for (int i0 = 0; i0 < K && !full; i0 += NMS_AHEAD) {
#pragma unroll
        for (int d = 0; d < NMS_AHEAD; ++d) {
            const int i = i0 + d;
            if (i >= K || full) continue;
            const unsigned long long row = ahead[d];
            ahead[d] = (mine && i + NMS_AHEAD < K) ? mask[(int64_t)(i + NMS_AHEAD) * NMS_WORDS + lane] : 0ull;
            const unsigned long long w = __shfl(removed, i >> 6);
            if ((w >> (i & 63)) & 1ull) continue;
            if (lane == 0) keep[n] = order[i];
            ++n;
            if (n == post_max) { full = true; continue; }
            // words left of the diagonal tile are never written by nms_mask_kernel and never used
            if (lane >= (i >> 6)) removed |= row;
        }
    }
    if (lane == 0) *count = n;
}

static int64_t nms_ws_order(int64_t N) { return al3d_align((N > NMS_MAX ? N : 0) * 4, 256); }

extern "C" int64_t al3d_nms_boxes_workspace_bytes(int64_t N)
{
    if (N < 0 || N >= (1LL << 31)) return -1;
    return 256 + nms_ws_order(N) + al3d_align(NMS_MAX * 4, 256) + (int64_t)NMS_MAX * NMS_WORDS * 8;
}

extern "C" int al3d_nms_boxes_launch_f32(const float* boxes, const float* scores, int64_t N, int box_dim, int rot_col, int layout,
                                         int convention, int mode, float thresh, int pre_max, int post_max, int* keep,
                                         int64_t keep_cap, int* count, void* workspace, int sort_threads, int mask_threads,
                                         int reject, void* stream)
{
    const char* who = "al3d_nms_boxes_f32";
    AL3D_REQUIRE(N >= 0 && N < (1LL << 31), "%s: bad sizes", who);
    if (box_format_check(who, box_dim, rot_col, layout, convention, AL3D_IOU_H_NONE)) return AL3D_EINVAL;
    AL3D_REQUIRE(mode == AL3D_NMS_ROTATED || mode == AL3D_NMS_NORMAL, "%s: bad mode", who);
    AL3D_REQUIRE(thresh == thresh, "%s: thresh is NaN", who);
    AL3D_REQUIRE((sort_threads == 256 || sort_threads == 1024) && (mask_threads == 64 || mask_threads == 128 || mask_threads == 256),
                 "%s: 256 or 1024 sort threads and 64, 128 or 256 mask threads", who);
    const int64_t K = pre_max > 0 && pre_max < N ? pre_max : N;
    AL3D_REQUIRE(K <= NMS_MAX, "%s: %lld candidates after pre_max, at most %d (AL3D_NMS_MAX_CANDIDATES)", who, (long long)K, NMS_MAX);
    const int64_t most = post_max > 0 && post_max < K ? post_max : K;
    AL3D_REQUIRE(keep_cap >= most, "%s: keep holds %lld of %lld indices", who, (long long)keep_cap, (long long)most);
    AL3D_REQUIRE(count, "%s: null pointer", who);
    hipStream_t st = (hipStream_t)stream;
    if (K == 0) {
        if (hipMemsetAsync(count, 0, sizeof(int), st) != hipSuccess) return al3d_fail(AL3D_ELAUNCH, "%s: memset", who);
        return AL3D_OK;
    }
    AL3D_REQUIRE(boxes && scores && keep && workspace, "%s: null pointer", who);
    char* ws = (char*)al3d_align((int64_t)(uintptr_t)workspace, 256);
    unsigned* keys = (unsigned*)ws;
    int* order = (int*)(ws + nms_ws_order(N));
    unsigned long long* mask = (unsigned long long*)((char*)order + al3d_align(NMS_MAX * 4, 256));
    if (sort_threads == 1024)
        hipLaunchKernelGGL(nms_order_kernel<1024>, dim3(1), dim3(1024), 0, st, scores, (int)N, (int)K, keys, order);
    else
        hipLaunchKernelGGL(nms_order_kernel<256>, dim3(1), dim3(256), 0, st, scores, (int)N, (int)K, keys, order);
    AL3D_CHECK_LAUNCH("nms_order_kernel");
    const BoxFormat f = {box_dim, rot_col, layout, convention, AL3D_IOU_H_NONE};
    const unsigned tiles = (unsigned)al3d_cdiv(K, BOX_TILE);
    hipLaunchKernelGGL(nms_mask_kernel, dim3(tiles, tiles), dim3(mask_threads), 0, st, boxes, f, order, (int)K, mode, thresh,
                       reject ? 1 : 0, mask);
    AL3D_CHECK_LAUNCH("nms_mask_kernel");
    hipLaunchKernelGGL(nms_walk_kernel, dim3(1), dim3(64), 0, st, mask, order, (int)K, post_max > 0 ? post_max : -1, keep, count);
    AL3D_CHECK_LAUNCH("nms_walk_kernel");
    return AL3D_OK;
}

extern "C" int al3d_nms_boxes_f32(const float* boxes, const float* scores, int64_t N, int box_dim, int rot_col, int layout,
                                  int convention, int mode, float thresh, int pre_max, int post_max, int* keep, int64_t keep_cap,
                                  int* count, void* workspace, void* stream)
{
    return al3d_nms_boxes_launch_f32(boxes, scores, N, box_dim, rot_col, layout, convention, mode, thresh, pre_max, post_max, keep,
                                     keep_cap, count, workspace, 1024, 256, 1, stream);
}
