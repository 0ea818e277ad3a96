// Train-mode Preprocess on the device (reference det3d/datasets/pipelines/preprocess.py:163-247 over
// det3d/core/sampler/preprocess.py): the per-object noise search and ONE fused pass over the points.
//
// (a) aug_noise_kernel -- noise_per_box (sampler/preprocess.py:238-267) with box_collision_test (:876-959), one workgroup
//     per frame.  Boxes run strictly in row order (a success overwrites box_corners[i], later boxes test against it); inside
//     a box, `tile` tries at a time, every (try, other box) pair of the chunk on its own thread; a chunk's answer is its
//     smallest try without a hit, so the result does not depend on tile or threads.  Corners and their stand-up boxes
//     stay in LDS (R <= AL3D_AUG_MAX_BOXES).
// (b) aug_count_kernel / aug_points_kernel -- remove_points_after_sample (pipelines/preprocess.py:178-180), points_transform_
//     (sampler/preprocess.py:450-467), random_flip_both (:829-854), global_rotation (:796-813), global_scaling_v2
//     (:857-861), np.random.shuffle and symmetry_intensity (pipelines/preprocess.py:215-247) in one walk.  Membership is
//     the sign rule of points_in_boxes.hip on host-built planes.  Shape as there: grid = (groups, frames), every wave owns one
//     contiguous span of its frame's points; a point's rank among the kept ones = the scanned partial count of its span +
//     the ballot popcount of the lower lanes, so every row lands at the same place whatever the launch shape.
// Every product and sum is rounded to float32 on its own (__fmul_rn / __fadd_rn, -ffp-contract=off); the `+ loc` steps are
// evaluated in double and rounded once, like numpy's float32 += float64.  No float atomics.
#include "al3d_common.h"
#include "al3d_scan.h"

#define AUG_TILE 64                 // boxes in LDS at a time (point pass); tries per chunk at most (noise)
#define AUG_HDR_BYTES 256           // workspace header: int[0] = magic, [1] = slots, [2] = B
#define AUG_MAGIC 0x41554731        // "AUG1"

__device__ __forceinline__ bool aug_inside(const float4* __restrict__ pl, float x, float y, float z)
{
    bool in = true;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const float4 n = pl[k];
        const float sign = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(x, n.x), __fmul_rn(y, n.y)), __fmul_rn(z, n.z)), n.w);
        in = in && !(sign >= 0.f);
    }
    return in;
}

// ------------------------------------------------------------------------------------------------ (a) noise per box
// box_collision_test's body for one (box, qbox) pair; b / q = 4 corners (x, y), bs / qs = stand-up (xmin, ymin, xmax, ymax)
__device__ __forceinline__ bool aug_collide(const float* __restrict__ b, const float4 bs, const float* __restrict__ q,
                                            const float4 qs)
{
    const float iw = __fsub_rn(fminf(bs.z, qs.z), fmaxf(bs.x, qs.x));
    if (!(iw > 0.f)) return false;
    const float ih = __fsub_rn(fminf(bs.w, qs.w), fmaxf(bs.y, qs.y));
    if (!(ih > 0.f)) return false;
    for (int k = 0; k < 4; ++k) {
        const float A0 = b[2 * k], A1 = b[2 * k + 1], B0 = b[2 * ((k + 1) & 3)], B1 = b[2 * ((k + 1) & 3) + 1];
        for (int l = 0; l < 4; ++l) {
            const float C0 = q[2 * l], C1 = q[2 * l + 1], D0 = q[2 * ((l + 1) & 3)], D1 = q[2 * ((l + 1) & 3) + 1];
            const bool acd = __fmul_rn(__fsub_rn(D1, A1), __fsub_rn(C0, A0)) > __fmul_rn(__fsub_rn(C1, A1), __fsub_rn(D0, A0));
            const bool bcd = __fmul_rn(__fsub_rn(D1, B1), __fsub_rn(C0, B0)) > __fmul_rn(__fsub_rn(C1, B1), __fsub_rn(D0, B0));
            if (acd != bcd) {
                const bool abc = __fmul_rn(__fsub_rn(C1, A1), __fsub_rn(B0, A0)) > __fmul_rn(__fsub_rn(B1, A1), __fsub_rn(C0, A0));
                const bool abd = __fmul_rn(__fsub_rn(D1, A1), __fsub_rn(B0, A0)) > __fmul_rn(__fsub_rn(B1, A1), __fsub_rn(D0, A0));
                if (abc != abd) return true;
            }
        }
    }
    // complete overlap: every corner of q strictly inside b (clockwise: vec = -(b[k] - b[k+1]))
    bool b_over_q = true;
    for (int l = 0; l < 4 && b_over_q; ++l)
        for (int k = 0; k < 4; ++k) {
            const float v0 = -__fsub_rn(b[2 * k], b[2 * ((k + 1) & 3)]), v1 = -__fsub_rn(b[2 * k + 1], b[2 * ((k + 1) & 3) + 1]);
            float cross = __fmul_rn(v1, __fsub_rn(b[2 * k], q[2 * l]));
            cross = __fsub_rn(cross, __fmul_rn(v0, __fsub_rn(b[2 * k + 1], q[2 * l + 1])));
            if (cross >= 0.f) { b_over_q = false; break; }
        }
    if (b_over_q) return true;
    bool q_over_b = true;
    for (int l = 0; l < 4 && q_over_b; ++l)
        for (int k = 0; k < 4; ++k) {
            const float v0 = -__fsub_rn(q[2 * k], q[2 * ((k + 1) & 3)]), v1 = -__fsub_rn(q[2 * k + 1], q[2 * ((k + 1) & 3) + 1]);
            float cross = __fmul_rn(v1, __fsub_rn(q[2 * k], b[2 * l]));
            cross = __fsub_rn(cross, __fmul_rn(v0, __fsub_rn(q[2 * k + 1], b[2 * l + 1])));
            if (cross >= 0.f) { q_over_b = false; break; }
        }
    return q_over_b;
}

__device__ __forceinline__ float4 aug_standup(const float* __restrict__ c)
{
    return make_float4(fminf(fminf(c[0], c[2]), fminf(c[4], c[6])), fminf(fminf(c[1], c[3]), fminf(c[5], c[7])),
                       fmaxf(fmaxf(c[0], c[2]), fmaxf(c[4], c[6])), fmaxf(fmaxf(c[1], c[3]), fmaxf(c[5], c[7])));
}

__global__ __launch_bounds__(256) void aug_noise_kernel(
    const float* __restrict__ corners, const float* __restrict__ centres, const unsigned char* __restrict__ valid,
    const float* __restrict__ rot_cos, const float* __restrict__ rot_sin, const double* __restrict__ loc,
    const int* __restrict__ box_off, int R, int T, int tile, int* __restrict__ selected, int* __restrict__ status)
{
    __shared__ float s_c[AL3D_AUG_MAX_BOXES * 8];      // 32 KB: the frame's current corners
    __shared__ float4 s_su[AL3D_AUG_MAX_BOXES];        // 16 KB: their stand-up boxes
    __shared__ float s_cand[AUG_TILE * 8];
    __shared__ float4 s_csu[AUG_TILE];
    __shared__ int s_hit[AUG_TILE];
    __shared__ int s_found;

    const int b = blockIdx.x, tid = threadIdx.x;
    const int r0 = box_off[b], r1 = box_off[b + 1];
    int bad = 0;
    if (r0 < 0 || r1 < r0 || r1 > R) bad |= AL3D_AUG_BAD_BOX_OFF;
    else if (r1 - r0 > AL3D_AUG_MAX_BOXES) bad |= AL3D_AUG_TOO_MANY_BOXES;
    if (T < 1 || T > AL3D_AUG_MAX_TRIES) bad |= AL3D_AUG_BAD_TRIES;
    if (bad) {                                         // wave-uniform: the frame counts as empty
        if (tid == 0) atomicOr(status, bad);
        return;
    }
    const int nb = r1 - r0;
    for (int i = tid; i < nb * 8; i += blockDim.x) s_c[i] = corners[(int64_t)r0 * 8 + i];
    __syncthreads();
    for (int i = tid; i < nb; i += blockDim.x) s_su[i] = aug_standup(&s_c[i * 8]);
    __syncthreads();

    for (int i = 0; i < nb; ++i) {
        int found = -1;
        if (valid[r0 + i]) {                           // block-uniform
            const float cx = centres[(int64_t)(r0 + i) * 2], cy = centres[(int64_t)(r0 + i) * 2 + 1];
            for (int t0 = 0; t0 < T && found < 0; t0 += tile) {
                const int nt = min(tile, T - t0);
                if (tid == 0) s_found = -1;
                // the candidates of the chunk: (corner - centre) @ [[c, -s], [s, c]] + (centre + loc in double)
                for (int e = tid; e < nt * 4; e += blockDim.x) {
                    const int t = e >> 2, k = e & 3;
                    const int64_t n = (int64_t)(r0 + i) * T + t0 + t;
                    const float c = rot_cos[n], s = rot_sin[n];
                    const float x = __fsub_rn(s_c[i * 8 + 2 * k], cx), y = __fsub_rn(s_c[i * 8 + 2 * k + 1], cy);
                    const float xr = __fadd_rn(__fmul_rn(x, c), __fmul_rn(y, s));
                    const float yr = __fadd_rn(__fmul_rn(x, -s), __fmul_rn(y, c));
                    s_cand[t * 8 + 2 * k] = (float)((double)xr + ((double)cx + loc[n * 3]));
                    s_cand[t * 8 + 2 * k + 1] = (float)((double)yr + ((double)cy + loc[n * 3 + 1]));
                }
                for (int t = tid; t < nt; t += blockDim.x) s_hit[t] = 0;
                __syncthreads();
                for (int t = tid; t < nt; t += blockDim.x) s_csu[t] = aug_standup(&s_cand[t * 8]);
                __syncthreads();
                for (int e = tid; e < nt * nb; e += blockDim.x) {
                    const int t = e / nb, j = e - t * nb;
                    if (j != i && aug_collide(&s_cand[t * 8], s_csu[t], &s_c[j * 8], s_su[j])) s_hit[t] = 1;
                }
                __syncthreads();
                if (tid == 0)
                    for (int t = 0; t < nt; ++t)
                        if (!s_hit[t]) { s_found = t0 + t; break; }
                __syncthreads();
                found = s_found;
                if (found >= 0 && tid < 8) s_c[i * 8 + tid] = s_cand[(found - t0) * 8 + tid];
                __syncthreads();
                if (found >= 0 && tid == 0) s_su[i] = aug_standup(&s_c[i * 8]);
                __syncthreads();
            }
        }
        if (tid == 0) selected[r0 + i] = found;
    }
}

// ------------------------------------------------------------------------------------------------ (b) the point pass
__device__ __forceinline__ int aug_frame(const int64_t* __restrict__ point_off, const int64_t* __restrict__ sampled_off,
                                         int b, int64_t P, int64_t& p0, int64_t& n, int64_t& ns)
{
    int bad = 0;
    const int64_t q0 = point_off[b], q1 = point_off[b + 1];
    if (q0 < 0 || q1 < q0 || q1 > P) bad |= AL3D_AUG_BAD_POINT_OFF;
    else if (q1 - q0 >= (1LL << 31)) bad |= AL3D_AUG_FRAME_TOO_LARGE;
    const int64_t s = sampled_off ? sampled_off[b] : 0;
    if (!bad && (s < 0 || s > q1 - q0)) bad |= AL3D_AUG_BAD_SAMPLED_OFF;
    p0 = bad ? 0 : q0;
    n = bad ? 0 : q1 - q0;
    ns = bad ? 0 : s;
    return bad;
}

__device__ __forceinline__ int aug_boxes(const int* __restrict__ box_off, int b, int R, int& r0, int& nb)
{
    const int s0 = box_off ? box_off[b] : 0, s1 = box_off ? box_off[b + 1] : 0;
    const int bad = (s0 < 0 || s1 < s0 || s1 > R) ? AL3D_AUG_BAD_BOX_OFF : 0;
    r0 = bad ? 0 : s0;
    nb = bad ? 0 : s1 - s0;
    return bad;
}

// drop_mask[p] = a scene point inside any of its frame's drop boxes; part[b, slot] = kept points of the slot; kept[b] += it
__global__ __launch_bounds__(256) void aug_count_kernel(
    const float* __restrict__ points, int64_t P, int F, const int64_t* __restrict__ point_off,
    const int64_t* __restrict__ sampled_off, const float* __restrict__ planes, const int* __restrict__ box_off, int R,
    int tile, int* __restrict__ hdr, int* __restrict__ part, unsigned char* __restrict__ drop_mask, int* __restrict__ kept,
    int* __restrict__ status)
{
    __shared__ float4 s_pl[AUG_TILE * 6];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, W = blockDim.x >> 6;
    const int b = blockIdx.y, S = gridDim.x * W, slot = blockIdx.x * W + wave;
    if (blockIdx.x == 0 && b == 0 && threadIdx.x == 0) { hdr[0] = AUG_MAGIC; hdr[1] = S; hdr[2] = (int)gridDim.y; }

    int64_t p0, n, ns;
    int r0, nb;
    int bad = aug_frame(point_off, sampled_off, b, P, p0, n, ns);
    bad |= aug_boxes(box_off, b, R, r0, nb);
    if (bad) { n = 0; nb = 0; }
    const int64_t per = ((n + S - 1) / S + 63) / 64 * 64;
    const int64_t start = min(n, (int64_t)slot * per), end = min(n, start + per);
    int acc = 0;
    for (int64_t it = 0; it < per; it += 64) {             // the same trip count for every wave of the workgroup
        const int64_t i = start + it + lane;
        const bool live = i < end;
        const float* p = points + (p0 + (live ? i : 0)) * F;
        float x = 0.f, y = 0.f, z = 0.f;
        if (live) { x = p[0]; y = p[1]; z = p[2]; }
        bool drop = false;
        for (int t0 = 0; t0 < nb; t0 += tile) {
            const int tb = min(tile, nb - t0);
            if (nb > tile || it == 0) {                    // one tile: loaded once
                __syncthreads();
                for (int e = threadIdx.x; e < tb * 6; e += blockDim.x)
                    s_pl[e] = reinterpret_cast<const float4*>(planes)[(int64_t)(r0 + t0) * 6 + e];
                __syncthreads();
            }
            if (live && i >= ns)
                for (int j = 0; j < tb && !drop; ++j) drop = aug_inside(&s_pl[j * 6], x, y, z);
        }
        if (live) drop_mask[p0 + i] = drop ? 1 : 0;
        acc += __popcll(__ballot(live && !drop));
    }
    if (!bad && lane == 0) {
        part[(int64_t)b * S + slot] = acc;
        if (acc) atomicAdd(&kept[b], acc);
    }
    if (bad && threadIdx.x == 0) atomicOr(status, bad);
}

__global__ __launch_bounds__(256) void aug_points_kernel(
    const float* __restrict__ points, int64_t P, int F, const int64_t* __restrict__ point_off,
    const unsigned char* __restrict__ drop_mask, const int* __restrict__ hdr, const int* __restrict__ part,
    const float* __restrict__ planes, const int* __restrict__ box_off, int R, const unsigned char* __restrict__ valid,
    const float* __restrict__ centres, const float* __restrict__ rot_cos, const float* __restrict__ rot_sin,
    const double* __restrict__ loc, const int* __restrict__ selected, int T, const unsigned char* __restrict__ flip,
    const float* __restrict__ global_xf, int symmetry, const int64_t* __restrict__ out_off,
    const int* __restrict__ rows, float* __restrict__ out, int64_t out_rows, int* __restrict__ owner, int tile,
    int* __restrict__ status)
{
    __shared__ float4 s_pl[AUG_TILE * 6];
    __shared__ unsigned char s_valid[AUG_TILE];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, W = blockDim.x >> 6;
    const int b = blockIdx.y, S = gridDim.x * W, slot = blockIdx.x * W + wave;
    if (drop_mask && (hdr[0] != AUG_MAGIC || hdr[1] != S || hdr[2] != (int)gridDim.y)) {
        if (threadIdx.x == 0) atomicOr(status, AL3D_AUG_BAD_WORKSPACE);
        return;
    }
    int64_t p0, n, ns;
    int r0, nb;
    int bad = aug_frame(point_off, nullptr, b, P, p0, n, ns);
    bad |= aug_boxes(box_off, b, R, r0, nb);
    if (nb > 0 && (T < 1 || T > AL3D_AUG_MAX_TRIES)) bad |= AL3D_AUG_BAD_TRIES;
    const int64_t o0 = out_off[b], o1 = out_off[b + 1];
    if (o0 < 0 || o1 < o0 || o1 > out_rows) bad |= AL3D_AUG_BAD_ROWS;
    if (bad) { n = 0; nb = 0; }
    const int64_t nk = bad ? 0 : o1 - o0;
    const int64_t per = ((n + S - 1) / S + 63) / 64 * 64;
    const int64_t start = min(n, (int64_t)slot * per), end = min(n, start + per);
    int64_t rank = start;                                  // nothing dropped: a point's rank is its index
    if (drop_mask && !bad) rank = (int64_t)((unsigned)part[(int64_t)b * S + slot] - (unsigned)part[(int64_t)b * S]);
    const bool fy = !bad && flip && flip[b * 2], fx = !bad && flip && flip[b * 2 + 1];
    const float gc = bad ? 1.f : global_xf[b * 3], gs = bad ? 0.f : global_xf[b * 3 + 1], sc = bad ? 1.f : global_xf[b * 3 + 2];
    int flags = 0;

    for (int64_t it = 0; it < per; it += 64) {
        const int64_t i = start + it + lane;
        const bool live = i < end;
        const float* p = points + (p0 + (live ? i : 0)) * F;
        float x = 0.f, y = 0.f, z = 0.f;
        if (live) { x = p[0]; y = p[1]; z = p[2]; }
        int own = -1;
        for (int t0 = 0; t0 < nb; t0 += tile) {
            const int tb = min(tile, nb - t0);
            if (nb > tile || it == 0) {
                __syncthreads();
                for (int e = threadIdx.x; e < tb * 6; e += blockDim.x)
                    s_pl[e] = reinterpret_cast<const float4*>(planes)[(int64_t)(r0 + t0) * 6 + e];
                for (int e = threadIdx.x; e < tb; e += blockDim.x) s_valid[e] = valid[r0 + t0 + e];
                __syncthreads();
            }
            if (live)
                for (int j = 0; j < tb && own < 0; ++j)
                    if (s_valid[j] && aug_inside(&s_pl[j * 6], x, y, z)) own = t0 + j;   // "only apply first box's transform"
        }
        const bool keep = live && !(drop_mask && drop_mask[p0 + i]);
        const unsigned long long m = __ballot(keep);
        if (live && owner) owner[p0 + i] = own;
        if (keep) {
            if (own >= 0) {                                // points_transform_: -= c, @ rot_mat_T, += c, += loc (double)
                const int r = r0 + own;
                int sel = selected[r];
                if (sel < -1 || sel >= T) { sel = -1; flags |= AL3D_AUG_BAD_SELECTED; }
                float c = 1.f, s = 0.f;
                double l0 = 0.0, l1 = 0.0, l2 = 0.0;
                if (sel >= 0) {
                    const int64_t e = (int64_t)r * T + sel;
                    c = rot_cos[e]; s = rot_sin[e];
                    l0 = loc[e * 3]; l1 = loc[e * 3 + 1]; l2 = loc[e * 3 + 2];
                }
                const float cx = centres[(int64_t)r * 3], cy = centres[(int64_t)r * 3 + 1], cz = centres[(int64_t)r * 3 + 2];
                const float dx = __fsub_rn(x, cx), dy = __fsub_rn(y, cy), dz = __fsub_rn(z, cz);
                const float xr = __fadd_rn(__fadd_rn(__fmul_rn(dx, c), __fmul_rn(dy, s)), __fmul_rn(dz, 0.f));
                const float yr = __fadd_rn(__fadd_rn(__fmul_rn(dx, -s), __fmul_rn(dy, c)), __fmul_rn(dz, 0.f));
                const float zr = __fadd_rn(__fadd_rn(__fmul_rn(dx, 0.f), __fmul_rn(dy, 0.f)), __fmul_rn(dz, 1.f));
                x = (float)((double)__fadd_rn(xr, cx) + l0);
                y = (float)((double)__fadd_rn(yr, cy) + l1);
                z = (float)((double)__fadd_rn(zr, cz) + l2);
            }
            if (fy) y = -y;
            if (fx) x = -x;
            const float xg = __fadd_rn(__fadd_rn(__fmul_rn(x, gc), __fmul_rn(y, gs)), __fmul_rn(z, 0.f));
            const float yg = __fadd_rn(__fadd_rn(__fmul_rn(x, -gs), __fmul_rn(y, gc)), __fmul_rn(z, 0.f));
            const float zg = __fadd_rn(__fadd_rn(__fmul_rn(x, 0.f), __fmul_rn(y, 0.f)), __fmul_rn(z, 1.f));
            const int64_t k = rank + __popcll(m & ((1ull << lane) - 1ull));
            int64_t row = -1;
            if (k >= 0 && k < nk) {
                row = rows ? (int64_t)rows[o0 + k] : k;
                if (row < 0 || row >= nk) row = -1;
            }
            if (row >= 0) {
                float* o = out + (o0 + row) * F;
                o[0] = __fmul_rn(xg, sc);
                o[1] = __fmul_rn(yg, sc);
                o[2] = __fmul_rn(zg, sc);
                for (int c = 3; c < F; ++c) o[c] = p[c];
                if (symmetry) o[F - 1] = __fsub_rn(o[F - 1], 0.5f);
            } else {
                flags |= AL3D_AUG_BAD_ROWS;
            }
        }
        rank += __popcll(m);
    }
    if (bad && threadIdx.x == 0) atomicOr(status, bad);
    if (flags) atomicOr(status, flags);
}

// ------------------------------------------------------------------------------------------------ host entries
static bool aug_shape_ok(int groups, int threads, int tile)
{
    return groups >= 1 && groups <= 1024 && (threads == 64 || threads == 128 || threads == 256) && tile >= 1 &&
           tile <= AUG_TILE;
}

static int64_t aug_part_bytes(int64_t B, int64_t slots) { return al3d_align(B * slots * 4, 256); }

extern "C" int64_t al3d_augment_points_workspace_bytes(int B, int groups, int threads)
{
    if (B < 0 || B >= 65536 || !aug_shape_ok(groups, threads, 1)) return -1;
    const int64_t slots = (int64_t)groups * (threads / 64);
    return AUG_HDR_BYTES + aug_part_bytes(B, slots) + al3d_scan_workspace_bytes((int64_t)B * slots);
}

extern "C" int al3d_noise_per_box_launch_f32(const float* corners, const float* centres, const unsigned char* valid_mask,
                                             const float* rot_cos, const float* rot_sin, const double* loc_noises,
                                             const int* box_off, int B, int R, int T, int* selected, int* status,
                                             int groups, int threads, int tile, void* stream)
{
    const char* who = "al3d_noise_per_box_f32";
    AL3D_REQUIRE(B >= 0 && B < 65536 && R >= 0, "%s: bad sizes", who);
    AL3D_REQUIRE(aug_shape_ok(groups, threads, tile), "%s: groups in [1, 1024], threads 64 / 128 / 256, tile in [1, 64]", who);
    AL3D_REQUIRE(status, "%s: null pointer", who);
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(status, 0, sizeof(int), st) != hipSuccess) return al3d_fail(AL3D_ELAUNCH, "%s: memset", who);
    if (B == 0) return AL3D_OK;
    AL3D_REQUIRE(box_off, "%s: null pointer", who);
    AL3D_REQUIRE(R == 0 || (corners && centres && valid_mask && rot_cos && rot_sin && loc_noises && selected),
                 "%s: null pointer", who);
    // one workgroup per frame: `groups` has no say here and is only checked
    hipLaunchKernelGGL(aug_noise_kernel, dim3((unsigned)B), dim3((unsigned)threads), 0, st, corners, centres, valid_mask,
                       rot_cos, rot_sin, loc_noises, box_off, R, T, tile, selected, status);
    AL3D_CHECK_LAUNCH("aug_noise_kernel");
    return AL3D_OK;
}

extern "C" int al3d_noise_per_box_f32(const float* corners, const float* centres, const unsigned char* valid_mask,
                                      const float* rot_cos, const float* rot_sin, const double* loc_noises,
                                      const int* box_off, int B, int R, int T, int* selected, int* status, void* stream)
{
    return al3d_noise_per_box_launch_f32(corners, centres, valid_mask, rot_cos, rot_sin, loc_noises, box_off, B, R, T,
                                         selected, status, 1, AL3D_AUG_THREADS, AL3D_AUG_NOISE_TILE, stream);
}

static int aug_check(const char* who, const float* points, int64_t P, int F, const int64_t* point_off, int B, int R,
                     const int* status, int groups, int threads, int tile)
{
    AL3D_REQUIRE(P >= 0 && F >= 3 && B >= 0 && B < 65536 && R >= 0, "%s: bad sizes", who);
    AL3D_REQUIRE(aug_shape_ok(groups, threads, tile), "%s: groups in [1, 1024], threads 64 / 128 / 256, tile in [1, 64]", who);
    AL3D_REQUIRE(status, "%s: null pointer", who);
    if (B == 0) return AL3D_OK;
    AL3D_REQUIRE(point_off, "%s: null pointer", who);
    AL3D_REQUIRE(P == 0 || points, "%s: null pointer", who);
    return AL3D_OK;
}

extern "C" int al3d_augment_points_count_launch_f32(const float* points, int64_t P, int F, const int64_t* point_off,
                                                    const int64_t* sampled_off, int B, const float* drop_planes,
                                                    const int* drop_off, int R, unsigned char* drop_mask, int* kept,
                                                    void* workspace, int* status, int groups, int threads, int tile,
                                                    void* stream)
{
    const char* who = "al3d_augment_points_count_f32";
    const int rc = aug_check(who, points, P, F, point_off, B, R, status, groups, threads, tile);
    if (rc != AL3D_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(status, 0, sizeof(int), st) != hipSuccess) return al3d_fail(AL3D_ELAUNCH, "%s: memset", who);
    if (B == 0) return AL3D_OK;
    AL3D_REQUIRE(sampled_off && kept && workspace, "%s: null pointer", who);
    AL3D_REQUIRE(P == 0 || drop_mask, "%s: null pointer", who);
    AL3D_REQUIRE(R == 0 || (drop_planes && drop_off), "%s: null pointer", who);
    const int64_t slots = (int64_t)groups * (threads / 64);
    int* hdr = (int*)workspace;
    int* part = (int*)((char*)workspace + AUG_HDR_BYTES);
    void* scan_ws = (char*)workspace + AUG_HDR_BYTES + aug_part_bytes(B, slots);
    // a frame with bad offsets writes nothing: zero its counts, the scan reads every one
    if (hipMemsetAsync(part, 0, (size_t)aug_part_bytes(B, slots), st) != hipSuccess ||
        hipMemsetAsync(kept, 0, (size_t)B * sizeof(int), st) != hipSuccess)
        return al3d_fail(AL3D_ELAUNCH, "%s: memset", who);
    hipLaunchKernelGGL(aug_count_kernel, dim3((unsigned)groups, (unsigned)B), dim3((unsigned)threads), 0, st, points, P, F,
                       point_off, sampled_off, drop_planes, R ? drop_off : (const int*)nullptr, R, tile, hdr, part, drop_mask,
                       kept, status);
    AL3D_CHECK_LAUNCH("aug_count_kernel");
    return al3d_exclusive_scan_i32(part, part, (int64_t)B * slots, scan_ws, st);
}

extern "C" int al3d_augment_points_count_f32(const float* points, int64_t P, int F, const int64_t* point_off,
                                             const int64_t* sampled_off, int B, const float* drop_planes, const int* drop_off,
                                             int R, unsigned char* drop_mask, int* kept, void* workspace, int* status,
                                             void* stream)
{
    return al3d_augment_points_count_launch_f32(points, P, F, point_off, sampled_off, B, drop_planes, drop_off, R, drop_mask,
                                                kept, workspace, status, AL3D_AUG_GROUPS, AL3D_AUG_THREADS, AUG_TILE, stream);
}

extern "C" int al3d_augment_points_launch_f32(const float* points, int64_t P, int F, const int64_t* point_off, int B,
                                              const unsigned char* drop_mask, const void* workspace, const float* planes,
                                              const int* box_off, int R, const unsigned char* valid_mask,
                                              const float* centres, const float* rot_cos, const float* rot_sin,
                                              const double* loc_noises, const int* selected, int T,
                                              const unsigned char* flip, const float* global_xf, int symmetry,
                                              const int64_t* out_off, const int* rows, float* out, int64_t out_rows,
                                              int* owner, int* status, int groups, int threads, int tile, void* stream)
{
    const char* who = "al3d_augment_points_f32";
    const int rc = aug_check(who, points, P, F, point_off, B, R, status, groups, threads, tile);
    if (rc != AL3D_OK) return rc;
    AL3D_REQUIRE(out_rows >= 0, "%s: bad sizes", who);
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(status, 0, sizeof(int), st) != hipSuccess) return al3d_fail(AL3D_ELAUNCH, "%s: memset", who);
    if (B == 0) return AL3D_OK;
    AL3D_REQUIRE(global_xf && out_off, "%s: null pointer", who);
    AL3D_REQUIRE(out_rows == 0 || out, "%s: null pointer", who);
    AL3D_REQUIRE(!drop_mask || workspace, "%s: a drop mask needs the count entry's workspace", who);
    AL3D_REQUIRE(R == 0 || (planes && box_off && valid_mask && centres && rot_cos && rot_sin && loc_noises && selected),
                 "%s: null pointer", who);
    const int* hdr = (const int*)workspace;
    const int* part = workspace ? (const int*)((const char*)workspace + AUG_HDR_BYTES) : nullptr;
    hipLaunchKernelGGL(aug_points_kernel, dim3((unsigned)groups, (unsigned)B), dim3((unsigned)threads), 0, st, points, P, F,
                       point_off, drop_mask, hdr, part, planes, R ? box_off : (const int*)nullptr, R, valid_mask, centres,
                       rot_cos, rot_sin, loc_noises, selected, T, flip, global_xf, symmetry, out_off, rows, out, out_rows,
                       owner, tile, status);
    AL3D_CHECK_LAUNCH("aug_points_kernel");
    return AL3D_OK;
}

extern "C" int al3d_augment_points_f32(const float* points, int64_t P, int F, const int64_t* point_off, int B,
                                       const unsigned char* drop_mask, const void* workspace, const float* planes,
                                       const int* box_off, int R, const unsigned char* valid_mask, const float* centres,
                                       const float* rot_cos, const float* rot_sin, const double* loc_noises,
                                       const int* selected, int T, const unsigned char* flip, const float* global_xf,
                                       int symmetry, const int64_t* out_off, const int* rows, float* out, int64_t out_rows,
                                       int* owner, int* status, void* stream)
{
    return al3d_augment_points_launch_f32(points, P, F, point_off, B, drop_mask, workspace, planes, box_off, R, valid_mask,
                                          centres, rot_cos, rot_sin, loc_noises, selected, T, flip, global_xf, symmetry,
                                          out_off, rows, out, out_rows, owner, status, AL3D_AUG_GROUPS, AL3D_AUG_THREADS,
                                          AUG_TILE, stream);
}
