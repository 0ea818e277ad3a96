// The PPAL / CALD pre-passes (reference tools/ppal_pred_list.py + ppal_unc.py, tools/cald_pred_list.py + cald_ent.py):
// the nuScenes matching rule of classwise_weight/algo.py:36-106 on the raw NMS buffers, and the augmented view CALD
// compares against (det3d/core/sampler/preprocess.py:787-854: flip, rotation, scaling of the points).
//
// match_boxes_kernel: one 64-lane workgroup per (class, frame).  Classes are independent and the greedy is sequential only
// inside a class, so the workgroup gathers its class's predictions and reference rows into LDS (order kept), sorts the
// (score, position) keys there and walks them: all lanes scan the class's free reference rows strided, a wave reduction
// takes the lexicographic minimum of (distance, row), lane 0 records the match.  Latency-bound like head_nms.hip.
#include "al3d_common.h"

#define MATCH_MAX_PRED 512      // predictions of one class in one frame (sort keys in LDS)
#define MATCH_MAX_REF 1024      // reference rows of one class in one frame (taken bits in LDS)

struct MatchView { float flip_x, flip_y, c, s, scale; };   // c, s: cos / sin of the view's rotation

// score -> unsigned with the same order (IEEE totalOrder on non-NaN values)
__device__ __forceinline__ unsigned match_score_key(float v)
{
    const unsigned u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// a prediction's xy centre mapped back through the inverse of the view: un-scale, un-rotate, un-flip
// (the forward view is x' = c x + s y, y' = -s x + c y: det3d's rotation_points_single_angle(axis=2))
__device__ __forceinline__ void match_unview(const MatchView& v, float& x, float& y)
{
    const float xs = x / v.scale, ys = y / v.scale;
    x = (v.c * xs - v.s * ys) * v.flip_y;
    y = (v.s * xs + v.c * ys) * v.flip_x;
}

__global__ __launch_bounds__(64) void match_boxes_kernel(
    const float* __restrict__ boxes, const float* __restrict__ scores, const int* __restrict__ labels,
    const int* __restrict__ counts, int nt, int post, int box_dim, const float* __restrict__ ref_boxes,
    const int* __restrict__ ref_labels, const float* __restrict__ ref_scores, const int* __restrict__ ref_off, int R,
    int ref_dim, int ncls, float dist_th, int max_boxes, const float* __restrict__ class_range,
    const float* __restrict__ origin, int has_view, MatchView view, int* __restrict__ match_ref,
    float* __restrict__ match_iou, int* __restrict__ cls_count, float* __restrict__ cls_quality,
    float* __restrict__ cls_cons, int* __restrict__ status)
{
    __shared__ unsigned long long s_key[MATCH_MAX_PRED];
    __shared__ float s_px[MATCH_MAX_PRED], s_py[MATCH_MAX_PRED];
    __shared__ int s_pslot[MATCH_MAX_PRED];              // t * post + i of the gathered prediction
    __shared__ float s_rx[MATCH_MAX_REF], s_ry[MATCH_MAX_REF];
    __shared__ int s_rrow[MATCH_MAX_REF];
    __shared__ unsigned long long s_taken[MATCH_MAX_REF / 64];

    const int c = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
    const int64_t fbase = (int64_t)b * nt * post;        // the frame's first slot
    const float ox = origin ? origin[2 * b] : 0.f, oy = origin ? origin[2 * b + 1] : 0.f;
    const float range = class_range ? class_range[c] : 0.f;
    int bad = 0;

    // a class without a match keeps these (cald_ent.py:73-89 seeds the consistency with 1.0)
    int n_match = 0;
    float quality = 0.f, cons = 1.0f;

    // ---- the frame's size (load_prediction's limit counts every valid prediction, before any filter)
    int total = 0;
    for (int t = 0; t < nt; ++t) total += min(max(counts[b * nt + t], 0), post);
    if (total > max_boxes) bad |= AL3D_MATCH_TOO_MANY_BOXES;

    // ---- gather the class's reference rows, ascending row index
    int r0 = ref_off[b], r1 = ref_off[b + 1];
    if (r0 < 0 || r1 < r0 || r1 > R) { bad |= AL3D_MATCH_BAD_OFFSETS; r0 = r1 = 0; }
    int nref = 0;
    for (int base = r0; base < r1; base += 64) {
        const int r = base + lane;
        bool keep = false;
        float x = 0.f, y = 0.f;
        if (r < r1 && ref_labels[r] == c) {
            x = ref_boxes[(int64_t)r * ref_dim];
            y = ref_boxes[(int64_t)r * ref_dim + 1];
            keep = true;
            if (class_range) {
                const float dx = x - ox, dy = y - oy;
                keep = !(sqrtf(dx * dx + dy * dy) >= range);
            }
        }
        const unsigned long long m = __ballot(keep);
        const int at = nref + __popcll(m & ((1ull << lane) - 1ull));
        if (keep && at < MATCH_MAX_REF) { s_rx[at] = x; s_ry[at] = y; s_rrow[at] = r; }
        nref += __popcll(m);
    }
    if (nref > MATCH_MAX_REF) { bad |= AL3D_MATCH_CLASS_TOO_LARGE; nref = 0; }
    if (lane < MATCH_MAX_REF / 64) s_taken[lane] = 0ull;

    // ---- gather the class's predictions in the frame's concatenated order (task-major, then slot)
    int npred = 0;
    for (int t = 0; t < nt; ++t) {
        const int cnt = min(max(counts[b * nt + t], 0), post);
        for (int base = 0; base < cnt; base += 64) {
            const int i = base + lane;
            bool keep = false;
            float x = 0.f, y = 0.f;
            const int64_t o = fbase + (int64_t)t * post + i;
            if (i < cnt && labels[o] == c) {
                x = boxes[o * box_dim];
                y = boxes[o * box_dim + 1];
                if (has_view) match_unview(view, x, y);
                keep = true;
                if (class_range) {
                    const float dx = x - ox, dy = y - oy;
                    keep = !(sqrtf(dx * dx + dy * dy) >= range);
                }
            }
            const unsigned long long m = __ballot(keep);
            const int at = npred + __popcll(m & ((1ull << lane) - 1ull));
            if (keep && at < MATCH_MAX_PRED) {
                s_px[at] = x; s_py[at] = y; s_pslot[at] = t * post + i;
                s_key[at] = ((unsigned long long)match_score_key(scores[o]) << 32) | (unsigned)at;
            }
            npred += __popcll(m);
        }
    }
    if (npred > MATCH_MAX_PRED) { bad |= AL3D_MATCH_CLASS_TOO_LARGE; npred = 0; }

    // ---- descending (score, position): sorted((v, i))[::-1] of algo.py:54.  Bitonic, padded with zero keys (they sort last)
    int np2 = 1;
    while (np2 < npred) np2 <<= 1;
    for (int i = npred + lane; i < np2; i += 64) s_key[i] = 0ull;
    __syncthreads();
    for (int size = 2; size <= np2; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int i = lane; i < np2; i += 64) {
                const int j = i ^ stride;
                if (j > i) {
                    const bool desc = (i & size) == 0;
                    const unsigned long long a = s_key[i], k = s_key[j];
                    if (desc ? a < k : a > k) { s_key[i] = k; s_key[j] = a; }
                }
            }
            __syncthreads();
        }

    // ---- the greedy walk (algo.py:70-106)
    for (int k = 0; k < npred && nref > 0; ++k) {
        const int g = (int)(s_key[k] & 0xffffffffull);
        const float px = s_px[g], py = s_py[g];
        float best = __builtin_inff();
        int best_j = 0x7fffffff;
        for (int j = lane; j < nref; j += 64) {
            if ((s_taken[j >> 6] >> (j & 63)) & 1ull) continue;
            const float dx = s_rx[j] - px, dy = s_ry[j] - py;
            const float d2 = dx * dx + dy * dy;
            if (d2 < best) { best = d2; best_j = j; }      // strictly smaller: the lane's earliest row keeps a tie
        }
        for (int off = 32; off > 0; off >>= 1) {           // lexicographic minimum of (distance, row) on every lane
            const float od = __shfl_xor(best, off);
            const int oj = __shfl_xor(best_j, off);
            if (od < best || (od == best && oj < best_j)) { best = od; best_j = oj; }
        }
        if (best_j != 0x7fffffff && sqrtf(best) < dist_th) {
            const int row = s_rrow[best_j];
            const int64_t o = fbase + s_pslot[g];
            // the devkit's scale_iou: both boxes aligned, prod(min sizes) / (vol_a + vol_b - that)
            const float* pb = boxes + o * box_dim + 3;
            const float* rb = ref_boxes + (int64_t)row * ref_dim + 3;
            const float sc = has_view ? view.scale : 1.0f;
            const float pw = pb[0] / sc, pl = pb[1] / sc, ph = pb[2] / sc;
            const float rw = rb[0], rl = rb[1], rh = rb[2];
            const float inter = fminf(pw, rw) * fminf(pl, rl) * fminf(ph, rh);
            const float iou = inter / (pw * pl * ph + rw * rl * rh - inter);
            const float q = scores[o], p = ref_scores[row];
            // ppal_unc.py:76
            quality += powf(q, 0.6f) * powf(iou, 0.4f);
            // cald_ent.py:81-88.  Its js term is 0.5 entropy(p, m) + 0.5 entropy(q, m) of two SCALARS, and scipy's
            // entropy normalises each argument to sum 1: both are entropy(1, 1) = 0, so (1 - js) is identically 1
            cons = fminf(cons, fabsf(iou + 0.5f * (p + q) - 1.3f));
            ++n_match;
            if (lane == 0) {
                match_ref[o] = row;
                match_iou[o] = iou;
                s_taken[best_j >> 6] |= 1ull << (best_j & 63);
            }
            __syncthreads();
        }
    }
    if (lane == 0) {
        cls_count[b * ncls + c] = n_match;
        cls_quality[b * ncls + c] = quality;
        cls_cons[b * ncls + c] = cons;
        if (bad) atomicOr(status, bad);
    }
}

extern "C" int al3d_match_boxes_f32(const float* boxes, const float* scores, const int* labels, const int* counts, int B,
                                    int nt, int post, int box_dim, const float* ref_boxes, const int* ref_labels,
                                    const float* ref_scores, const int* ref_off, int R, int ref_dim, int ncls,
                                    float dist_th, int max_boxes, const float* class_range, const float* origin,
                                    const float* view, int* match_ref, float* match_iou, int* cls_count,
                                    float* cls_quality, float* cls_cons, int* status, void* stream)
{
    AL3D_REQUIRE(B >= 0 && nt >= 1 && post >= 1 && box_dim >= 6 && ref_dim >= 6 && R >= 0 && ncls >= 1 && max_boxes >= 0,
                 "al3d_match_boxes_f32: bad sizes");
    AL3D_REQUIRE((int64_t)B * nt * post < (1LL << 31) / box_dim && (int64_t)nt * post < (1LL << 31) && B < 65536,
                 "al3d_match_boxes_f32: batch too large");
    AL3D_REQUIRE(!(class_range && !origin), "al3d_match_boxes_f32: class_range needs origin");
    AL3D_REQUIRE(status, "al3d_match_boxes_f32: null pointer");
    MatchView v = {1.f, 1.f, 1.f, 0.f, 1.f};
    if (view) {
        AL3D_REQUIRE(view[3] > 0.f && view[3] == view[3] && view[2] == view[2], "al3d_match_boxes_f32: bad view");
        v.flip_x = view[0] != 0.f ? -1.f : 1.f;
        v.flip_y = view[1] != 0.f ? -1.f : 1.f;
        v.c = (float)cos((double)view[2]);
        v.s = (float)sin((double)view[2]);
        v.scale = view[3];
    }
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(status, 0, sizeof(int), st) != hipSuccess) return al3d_fail(AL3D_ELAUNCH, "al3d_match_boxes_f32: memset");
    if (B == 0) return AL3D_OK;
    AL3D_REQUIRE(boxes && scores && labels && counts && ref_off && match_ref && match_iou && cls_count && cls_quality &&
                 cls_cons, "al3d_match_boxes_f32: null pointer");
    AL3D_REQUIRE(R == 0 || (ref_boxes && ref_labels && ref_scores), "al3d_match_boxes_f32: null pointer");
    const size_t slots = (size_t)B * nt * post;
    if (hipMemsetAsync(match_ref, 0xff, slots * sizeof(int), st) != hipSuccess ||      // -1: no match
        hipMemsetAsync(match_iou, 0, slots * sizeof(float), st) != hipSuccess)
        return al3d_fail(AL3D_ELAUNCH, "al3d_match_boxes_f32: memset");
    hipLaunchKernelGGL(match_boxes_kernel, dim3((unsigned)ncls, (unsigned)B), dim3(64), 0, st, boxes, scores, labels, counts,
                       nt, post, box_dim, ref_boxes, ref_labels, ref_scores, ref_off, R, ref_dim, ncls, dist_th, max_boxes,
                       class_range, origin, view ? 1 : 0, v, match_ref, match_iou, cls_count, cls_quality, cls_cons, status);
    AL3D_CHECK_LAUNCH("match_boxes_kernel");
    return AL3D_OK;
}

// The augmented view of a point cloud, in place on the xyz columns of [P, F]: flip y if flip_x, flip x if flip_y (det3d's
// naming, preprocess.py:829-854), then rotate about z (x' = c x + s y, y' = -s x + c y, box_np_ops.py:396-418), then scale.
__global__ void points_view_kernel(float* __restrict__ pts, int64_t P, int F, float fx, float fy, float c, float s,
                                   float scale)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P) return;
    float* p = pts + i * F;
    const float x = p[0] * fy, y = p[1] * fx;
    p[0] = (c * x + s * y) * scale;
    p[1] = (c * y - s * x) * scale;
    p[2] = p[2] * scale;
}

extern "C" int al3d_points_view_f32(float* points, int64_t P, int F, int flip_x, int flip_y, float rot, float scale,
                                    void* stream)
{
    AL3D_REQUIRE(P >= 0 && F >= 3 && rot == rot && scale == scale, "al3d_points_view_f32: bad arguments");
    if (P == 0) return AL3D_OK;
    AL3D_REQUIRE(points, "al3d_points_view_f32: null pointer");
    AL3D_REQUIRE(al3d_cdiv(P, 256) < (1LL << 31), "al3d_points_view_f32: too many points");
    hipLaunchKernelGGL(points_view_kernel, dim3((unsigned)al3d_cdiv(P, 256)), dim3(256), 0, (hipStream_t)stream, points, P, F,
                       flip_x ? -1.f : 1.f, flip_y ? -1.f : 1.f, (float)cos((double)rot), (float)sin((double)rot), scale);
    AL3D_CHECK_LAUNCH("points_view_kernel");
    return AL3D_OK;
}
