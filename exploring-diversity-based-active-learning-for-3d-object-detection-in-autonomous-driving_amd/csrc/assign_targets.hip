// Anchor target assignment for a batch of labelled frames: the device form of AssignTarget's train branch
// (reference det3d/datasets/pipelines/preprocess.py:450-479 over TargetAssigner.assign_v2, target_assigner.py:68-142,
// create_target_np, target_ops.py:28-222 with positive_fraction=None / prune_anchor_fn=None / norm_by_num_examples=False,
// NearestIouSimilarity = iou_jit(eps=0) on near boxes, box_np_ops.py:957-996, and second_box_encode, :54-114).
//
// Shape.  One workgroup per (frame, anchor class) -- the launch entry may give fewer workgroups, which then walk the pairs
// with a grid stride.  Both global reductions of create_target_np are local to such a pair: the row argmax belongs to
// one anchor, the column maximum to one box of that class.  The [anchors, boxes] overlap matrix is never stored; it is
// computed twice:
//   walk 1: the class's boxes of the frame pass through LDS `chunk` at a time (wave 0 compacts the rows whose gt_class is
//           this class, in list order); every thread takes anchors tid, tid + threads, ... and raises the box's maximum
//           with an LDS atomicMax on the bit pattern (overlaps are >= 0, so the unsigned order is the float order; only
//           the rare positive overlaps that beat the value already there issue one).  The maxima go to gt_overlap [R].
//   walk 2: the same chunks again, now with their maxima; per anchor the running (max, first argmax) under a strict `>`
//           and `forced |= overlap == column max > 0`; then the labels, weights and the encoded box are written.
// With more than one chunk an anchor's (max, argmax, forced) between chunks waits in that anchor's own labels /
// reg_weights slots: the same thread writes and reads them, nothing else touches them before the final value lands.
// An exact max in any order is the same number, every anchor is owned by one thread, so the outputs are bit-identical
// for every groups / threads / chunk and from run to run.
//
// Arithmetic: iou_jit's float32 operations in its order, no contraction (__fmul_rn / __fadd_rn and -ffp-contract=off);
// the encode's + - * / sqrt are correctly rounded (`/` and sqrtf under hipcc's default IEEE divide and square root; the
// __fsqrt_rn of the HIP headers is the native approximation and is not used); logf / cosf / sinf are the device library's.
#include "al3d_common.h"

#define AT_MAX_FRAMES 256          // frames per launch: their offsets travel in the kernel arguments

struct AtArgs {
    al3d_assign_class_t cls[AL3D_ASSIGN_MAX_CLASSES];
    int gt_off[AT_MAX_FRAMES + 1];
    int num_classes, frames, frame0, chunk, norm_velo;
};

// box_np_ops.py:973-995 for one (anchor, box): area_a = (x2 - x0 + eps) * (y2 - y0 + eps), area_q likewise, eps = 0
__device__ __forceinline__ float at_iou(const float4 a, float area_a, const float4 q, float area_q)
{
    const float iw = __fsub_rn(fminf(a.z, q.z), fmaxf(a.x, q.x));
    if (iw > 0.f) {
        const float ih = __fsub_rn(fminf(a.w, q.w), fmaxf(a.y, q.y));
        if (ih > 0.f) {
            const float inter = __fmul_rn(iw, ih);
            const float ua = __fsub_rn(__fadd_rn(area_a, area_q), inter);
            return __fdiv_rn(inter, ua);
        }
    }
    return 0.f;
}

__device__ __forceinline__ float at_area(const float4 b)
{
    return __fmul_rn(__fadd_rn(__fsub_rn(b.z, b.x), 0.f), __fadd_rn(__fsub_rn(b.w, b.y), 0.f));
}

// second_box_encode (box_np_ops.py:54-114): g = the box, a = the anchor, o = code_size floats
template <int NDIM, bool VEC, bool LINEAR>
__device__ __forceinline__ void at_encode(const float* __restrict__ g, const float* __restrict__ a, bool norm_velo,
                                          float* __restrict__ o)
{
    const float xa = a[0], ya = a[1], za = a[2], wa = a[3], la = a[4], ha = a[5], ra = a[NDIM - 1];
    const float xg = g[0], yg = g[1], zg = g[2], wg = g[3], lg = g[4], hg = g[5], rg = g[NDIM - 1];
    const float diag = sqrtf(__fadd_rn(__fmul_rn(la, la), __fmul_rn(wa, wa)));
    o[0] = __fdiv_rn(__fsub_rn(xg, xa), diag);
    o[1] = __fdiv_rn(__fsub_rn(yg, ya), diag);
    o[2] = __fdiv_rn(__fsub_rn(zg, za), ha);
    const float lq = __fdiv_rn(lg, la), wq = __fdiv_rn(wg, wa), hq = __fdiv_rn(hg, ha);
    if (LINEAR) {
        o[3] = __fsub_rn(wq, 1.f); o[4] = __fsub_rn(lq, 1.f); o[5] = __fsub_rn(hq, 1.f);
    } else {
        o[3] = logf(wq); o[4] = logf(lq); o[5] = logf(hq);
    }
    int k = 6;
    if (NDIM == 9) {
        const float dvx = __fsub_rn(g[6], a[6]), dvy = __fsub_rn(g[7], a[7]);
        o[6] = norm_velo ? __fdiv_rn(dvx, diag) : dvx;
        o[7] = norm_velo ? __fdiv_rn(dvy, diag) : dvy;
        k = 8;
    }
    if (VEC) {
        o[k] = __fsub_rn(cosf(rg), cosf(ra));
        o[k + 1] = __fsub_rn(sinf(rg), sinf(ra));
    } else {
        o[k] = __fsub_rn(rg, ra);
    }
}

template <int NDIM, bool VEC, bool LINEAR>
__global__ __launch_bounds__(1024) void at_assign_kernel(
    const AtArgs args, const float* __restrict__ anchors, const float4* __restrict__ anchors_bv,
    const float* __restrict__ gt_boxes, const float4* __restrict__ gt_bv, const int* __restrict__ gt_class,
    int* __restrict__ labels, float* __restrict__ reg_targets, float* __restrict__ reg_weights, int* __restrict__ gt_index,
    float* __restrict__ gt_overlap)
{
    constexpr int CODE = NDIM + (VEC ? 1 : 0);
    __shared__ float4 s_bv[AL3D_ASSIGN_CHUNK];
    __shared__ float s_area[AL3D_ASSIGN_CHUNK];
    __shared__ int s_row[AL3D_ASSIGN_CHUNK];
    __shared__ unsigned s_cm[AL3D_ASSIGN_CHUNK];
    __shared__ int s_cnt, s_cursor;

    const int tid = threadIdx.x, lane = tid & 63, nthr = blockDim.x;
    const int chunk = args.chunk;
    const int pairs = args.frames * args.num_classes;

    for (int pair = blockIdx.x; pair < pairs; pair += gridDim.x) {
        const int fb = pair / args.num_classes, c = pair - fb * args.num_classes;
        const al3d_assign_class_t k = args.cls[c];
        const int g0 = args.gt_off[fb], n_raw = args.gt_off[fb + 1] - g0;
        const int n_anchor = k.num_loc * k.num_rot;
        // this frame's block of the task's [B, A_t] outputs
        const int64_t obase = k.out_base + (int64_t)(args.frame0 + fb) * k.task_anchors;

        // wave 0: the next (up to) `chunk` rows of this class from raw row `cursor` on, in list order
        auto stage = [&](int cursor, bool with_max) {
            __syncthreads();                               // the previous chunk has been read by every wave
            if (tid < 64) {
                int cnt = 0, cur = cursor;
                while (cnt < chunk && cur < n_raw) {
                    const int r = cur + lane;
                    const bool m = r < n_raw && gt_class[g0 + r] == c;
                    const unsigned long long mask = __ballot(m);
                    const int pos = cnt + __popcll(mask & ((1ull << lane) - 1ull));
                    const bool acc = m && pos < chunk;
                    if (acc) {
                        const float4 q = gt_bv[g0 + r];
                        s_bv[pos] = q;
                        s_area[pos] = at_area(q);
                        s_row[pos] = r;
                        s_cm[pos] = with_max ? __float_as_uint(gt_overlap[g0 + r]) : 0u;
                    }
                    const int total = __popcll(mask);
                    if (cnt + total <= chunk) {
                        cnt += total;
                        cur += 64;
                    } else {                               // the chunk filled up inside this step
                        const unsigned long long rej = mask & ~__ballot(acc);
                        cur += __ffsll((long long)rej) - 1;
                        cnt = chunk;
                    }
                }
                if (lane == 0) { s_cnt = cnt; s_cursor = min(cur, n_raw); }
            }
            __syncthreads();
        };

        // ---- walk 1: every box's maximum over the class's anchors
        int total = 0;
        for (int cursor = 0; cursor < n_raw;) {
            stage(cursor, false);
            const int cnt = s_cnt;
            cursor = s_cursor;
            total += cnt;
            if (cnt == 0) continue;                        // uniform
            for (int i = tid; i < n_anchor; i += nthr) {
                const float4 a = anchors_bv[k.anchor_begin + i];
                const float area_a = at_area(a);
                for (int j = 0; j < cnt; ++j) {
                    const float ov = at_iou(a, area_a, s_bv[j], s_area[j]);
                    if (ov > 0.f) {
                        const unsigned bits = __float_as_uint(ov);
                        if (bits > s_cm[j]) atomicMax(&s_cm[j], bits);
                    }
                }
            }
            __syncthreads();
            for (int j = tid; j < cnt; j += nthr) gt_overlap[g0 + s_row[j]] = __uint_as_float(s_cm[j]);
        }

        if (total == 0) {                                  // target_ops.py:163-164: a class without a box is all background
            for (int i = tid; i < n_anchor; i += nthr) {
                const int loc = i / k.num_rot;
                const int64_t o = obase + (int64_t)loc * k.slot_stride + k.slot_offset + (i - loc * k.num_rot);
                labels[o] = 0;
                reg_weights[o] = 0.f;
                if (gt_index) gt_index[o] = -1;
                for (int q = 0; q < CODE; ++q) reg_targets[o * CODE + q] = 0.f;
            }
            continue;
        }

        // ---- walk 2: row argmax, forced anchors, labels and the encoded boxes
        bool first = true;
        for (int cursor = 0; cursor < n_raw;) {
            stage(cursor, true);
            const int cnt = s_cnt;
            cursor = s_cursor;
            const bool last = cursor >= n_raw;
            for (int i = tid; i < n_anchor; i += nthr) {
                const int loc = i / k.num_rot;
                const int64_t o = obase + (int64_t)loc * k.slot_stride + k.slot_offset + (i - loc * k.num_rot);
                float best = -1.f;
                int arg = 0;
                bool forced = false;
                if (!first) {                              // parked by this thread after the previous chunk
                    best = reg_weights[o];
                    const int packed = labels[o];
                    arg = packed >> 1;
                    forced = packed & 1;
                }
                const float4 a = anchors_bv[k.anchor_begin + i];
                const float area_a = at_area(a);
                for (int j = 0; j < cnt; ++j) {
                    const float ov = at_iou(a, area_a, s_bv[j], s_area[j]);
                    if (ov > best) { best = ov; arg = s_row[j]; }
                    forced = forced || (ov > 0.f && __float_as_uint(ov) == s_cm[j]);
                }
                if (!last) {
                    reg_weights[o] = best;
                    labels[o] = (arg << 1) | (forced ? 1 : 0);
                    continue;
                }
                // target_ops.py:121-131, 163-168: forced, then >= matched, then < unmatched, then forced again
                const bool pos = best >= k.matched;
                const bool enc = pos || forced;            // fg_inds is taken before the background pass (:136)
                int label = -1;
                if (pos) label = k.label;
                if (best < k.unmatched) label = 0;
                if (forced) label = k.label;
                labels[o] = label;
                reg_weights[o] = label > 0 ? 1.f : 0.f;
                if (gt_index) gt_index[o] = enc ? arg : -1;
                float code[CODE];
                if (enc) {
                    at_encode<NDIM, VEC, LINEAR>(gt_boxes + (int64_t)(g0 + arg) * NDIM,
                                                 anchors + (int64_t)(k.anchor_begin + i) * NDIM, args.norm_velo != 0, code);
                } else {
#pragma unroll
                    for (int q = 0; q < CODE; ++q) code[q] = 0.f;
                }
#pragma unroll
                for (int q = 0; q < CODE; ++q) reg_targets[o * CODE + q] = code[q];
            }
            first = false;
        }
    }
}

typedef void (*at_kernel_t)(const AtArgs, const float*, const float4*, const float*, const float4*, const int*, int*,
                            float*, float*, int*, float*);

static at_kernel_t at_pick(int n_dim, int vec, int linear)
{
    if (n_dim == 7) {
        if (vec) return linear ? at_assign_kernel<7, true, true> : at_assign_kernel<7, true, false>;
        return linear ? at_assign_kernel<7, false, true> : at_assign_kernel<7, false, false>;
    }
    if (vec) return linear ? at_assign_kernel<9, true, true> : at_assign_kernel<9, true, false>;
    return linear ? at_assign_kernel<9, false, true> : at_assign_kernel<9, false, false>;
}

extern "C" int al3d_assign_targets_launch_f32(const float* anchors, const float* anchors_bv, int64_t A, int n_dim,
                                              const al3d_assign_class_t* classes, int num_classes, const float* gt_boxes,
                                              const float* gt_bv, const int* gt_class, int64_t R, const int* gt_off, int B,
                                              int vec_encode, int linear_dim, int norm_velo, int* labels, float* reg_targets,
                                              float* reg_weights, int* gt_index, int64_t out_rows, float* gt_overlap,
                                              int groups, int threads, int chunk, void* stream)
{
    const char* who = "al3d_assign_targets_f32";
    AL3D_REQUIRE(n_dim == 7 || n_dim == 9, "%s: n_dim must be 7 or 9, got %d", who, n_dim);
    AL3D_REQUIRE(A >= 0 && A < (1LL << 31) && R >= 0 && R < (1LL << 30) && B >= 0 && out_rows >= 0,
                 "%s: negative or oversized count (A %lld, R %lld, B %d, out_rows %lld)", who, (long long)A, (long long)R, B,
                 (long long)out_rows);
    AL3D_REQUIRE(num_classes >= 1 && num_classes <= AL3D_ASSIGN_MAX_CLASSES, "%s: num_classes in [1, %d] expected", who,
                 AL3D_ASSIGN_MAX_CLASSES);
    AL3D_REQUIRE(groups >= 1 && groups <= 65536 && threads >= 64 && threads <= 1024 && threads % 64 == 0 && chunk >= 1 &&
                     chunk <= AL3D_ASSIGN_CHUNK,
                 "%s: groups in [1, 65536], threads a multiple of 64 in [64, 1024], chunk in [1, %d]", who, AL3D_ASSIGN_CHUNK);
    AL3D_REQUIRE(classes, "%s: null pointer", who);
    for (int c = 0; c < num_classes; ++c) {
        const al3d_assign_class_t& k = classes[c];
        AL3D_REQUIRE(k.anchor_begin >= 0 && k.num_loc >= 0 && k.num_rot >= 1 &&
                         (int64_t)k.anchor_begin + (int64_t)k.num_loc * k.num_rot <= A,
                     "%s: class %d: anchors [%d, +%d x %d) overrun A = %lld", who, c, k.anchor_begin, k.num_loc, k.num_rot,
                     (long long)A);
        AL3D_REQUIRE(k.slot_offset >= 0 && k.slot_stride >= 1 && (int64_t)k.slot_offset + k.num_rot <= k.slot_stride &&
                         (int64_t)k.num_loc * k.slot_stride == k.task_anchors,
                     "%s: class %d: slot [%d, +%d) of %d per location, %d locations, task of %d anchors", who, c, k.slot_offset,
                     k.num_rot, k.slot_stride, k.num_loc, k.task_anchors);
        AL3D_REQUIRE(k.out_base >= 0 && k.out_base + (int64_t)B * k.task_anchors <= out_rows,
                     "%s: class %d: output block [%lld, +%d x %d) overruns out_rows = %lld", who, c, (long long)k.out_base, B,
                     k.task_anchors, (long long)out_rows);
        AL3D_REQUIRE(k.label >= 1, "%s: class %d: label %d (labels start at 1)", who, c, k.label);
    }
    if (B == 0) return AL3D_OK;
    AL3D_REQUIRE(gt_off, "%s: null pointer", who);
    AL3D_REQUIRE(gt_off[0] >= 0 && gt_off[B] <= R, "%s: gt_off must lie inside [0, R]", who);
    for (int b = 0; b < B; ++b)
        AL3D_REQUIRE(gt_off[b] <= gt_off[b + 1], "%s: gt_off must ascend (frame %d)", who, b);
    AL3D_REQUIRE(out_rows == 0 || (labels && reg_targets && reg_weights), "%s: null pointer", who);
    AL3D_REQUIRE(A == 0 || (anchors && anchors_bv), "%s: null pointer", who);
    AL3D_REQUIRE(R == 0 || (gt_boxes && gt_bv && gt_class && gt_overlap), "%s: null pointer", who);
    AL3D_REQUIRE(((uintptr_t)anchors_bv & 15) == 0 && ((uintptr_t)gt_bv & 15) == 0, "%s: anchors_bv / gt_bv must be 16-byte aligned",
                 who);

    hipStream_t st = (hipStream_t)stream;
    if (R > 0 && hipMemsetAsync(gt_overlap, 0, (size_t)R * sizeof(float), st) != hipSuccess)
        return al3d_fail(AL3D_ELAUNCH, "%s: memset", who);
    const at_kernel_t kern = at_pick(n_dim, vec_encode, linear_dim);
    AtArgs args;
    for (int c = 0; c < num_classes; ++c) args.cls[c] = classes[c];
    for (int c = num_classes; c < AL3D_ASSIGN_MAX_CLASSES; ++c) args.cls[c] = al3d_assign_class_t{};
    args.num_classes = num_classes;
    args.chunk = chunk;
    args.norm_velo = norm_velo ? 1 : 0;
    for (int f0 = 0; f0 < B; f0 += AT_MAX_FRAMES) {
        const int nf = B - f0 < AT_MAX_FRAMES ? B - f0 : AT_MAX_FRAMES;
        for (int b = 0; b <= AT_MAX_FRAMES; ++b) args.gt_off[b] = gt_off[f0 + (b < nf ? b : nf)];
        args.frames = nf;
        args.frame0 = f0;
        const int64_t pairs = (int64_t)nf * num_classes;
        hipLaunchKernelGGL(kern, dim3((unsigned)(pairs < groups ? pairs : groups)), dim3((unsigned)threads), 0, st, args, anchors,
                           (const float4*)anchors_bv, gt_boxes, (const float4*)gt_bv, gt_class, labels, reg_targets,
                           reg_weights, gt_index, gt_overlap);
        AL3D_CHECK_LAUNCH("at_assign_kernel");
    }
    return AL3D_OK;
}

extern "C" int al3d_assign_targets_f32(const float* anchors, const float* anchors_bv, int64_t A, int n_dim,
                                       const al3d_assign_class_t* classes, int num_classes, const float* gt_boxes,
                                       const float* gt_bv, const int* gt_class, int64_t R, const int* gt_off, int B,
                                       int vec_encode, int linear_dim, int norm_velo, int* labels, float* reg_targets,
                                       float* reg_weights, int* gt_index, int64_t out_rows, float* gt_overlap, void* stream)
{
    return al3d_assign_targets_launch_f32(anchors, anchors_bv, A, n_dim, classes, num_classes, gt_boxes, gt_bv, gt_class, R,
                                          gt_off, B, vec_encode, linear_dim, norm_velo, labels, reg_targets, reg_weights,
                                          gt_index, out_rows, gt_overlap, AL3D_ASSIGN_GROUPS, AL3D_ASSIGN_THREADS,
                                          AL3D_ASSIGN_CHUNK, stream);
}
