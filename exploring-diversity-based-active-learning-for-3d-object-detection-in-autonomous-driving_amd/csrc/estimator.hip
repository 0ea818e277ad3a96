// The box-wise IoU Estimator (reference det3d/models/detectors/estimator.py:22-105,155-274): for every predicted box the
// lidar points inside its doubled BEV footprint and its own height go through a three-layer PointNet, are max-pooled per
// box and a three-layer head turns the pooled row into the predicted IoU, which replaces the box's score; boxes without
// a point are dropped.  The reference builds a dense [points, boxes] mask per frame in chunks of 20 boxes and loops over
// the boxes in Python; here three launches, no host synchronisation:
//
//   est_prep_kernel   one wave per frame: checks the frame's point offsets and labels, gathers the valid boxes in the
//                     frame's task-major order and writes, per box, what the membership test reads: the four corners and
//                     edge vectors of the doubled footprint in the reference's own f32 operation order (corners_nd ->
//                     rotation_2d -> + centre, box_torch_ops.py:220-255,349-362,388-407), a reject radius, and sin / cos
//                     of the angle in double for the feature pass.
//   est_points_kernel one wave per 512 points of one frame.  Every lane tests its 8 points against each box of the frame
//                     (the box's record is wave-uniform: scalar loads); a radius reject, then the four strict cross
//                     products of geometry.py:5-31 and the inclusive height test.  Hits go to a per-wave queue in LDS.
//                     The queue is drained by the WHOLE wave, one hit at a time with the lanes as output channels: lane o
//                     holds row o of the (BatchNorm-folded) 32x(9+nc), 64x32 and two rows of the 128x64 weights in
//                     registers, the previous layer's activations reach it by v_readlane.  Consecutive hits of one box
//                     are max-reduced in registers, then 128 contiguous integer atomic max (outputs are post-ReLU, so
//                     >= 0, so ordered as unsigned) lower them into the box's pooled row.  Max and the integer point
//                     count do not depend on the order of arrival: the result is bit-identical from run to run.
//   est_head_kernel   one workgroup per (frame, task): stable compaction of the slots that hold a point, then the folded
//                     head (128 -> 256 -> 64 -> 1, sigmoid), four boxes per wave pass so a weight is loaded once for four.
//
// Built with -ffp-contract=off: the geometry's products and sums round separately, as torch's elementwise ops do.  The
// point network and the head accumulate their dot products in double on the vector ALUs (f32 weights and activations,
// explicit fma, one rounding per dot product); the sigmoid is taken in double and rounded once.  Independent of AL3D_MATH.
#include "al3d_common.h"

#define EST_PPL 8                        // points per lane
#define EST_WTILE (64 * EST_PPL)         // points per wave
#define EST_WAVES 4
#define EST_QCAP 1024                    // queue entries per wave; one box adds at most EST_WTILE
#define EST_C1 32
#define EST_C2 64
#define EST_C3 128
#define EST_H1 256
#define EST_H2 64
#define EST_TABB 18                      // floats per box: 4 corners (x, y), 4 edges (x, y), cz, h/2
#define EST_GROUP 4                      // boxes per wave pass of the head

struct EstWs { int* npts; unsigned* pooled; int* nbox; float4* tab_a; float* tab_b; double2* tab_c; };

static inline int64_t est_ws_layout(int B, int nt, int post, char* base, EstWs* w)
{
    const int64_t nb = (int64_t)nt * post, slots = (int64_t)B * nb;
    int64_t o = 0;
    if (w) w->npts = (int*)(base + o);
    o = al3d_align(o + slots * 4, 256);
    if (w) w->pooled = (unsigned*)(base + o);
    o = al3d_align(o + slots * EST_C3 * 4, 256);
    if (w) w->nbox = (int*)(base + o);
    o = al3d_align(o + (int64_t)B * 4, 256);
    if (w) w->tab_a = (float4*)(base + o);
    o = al3d_align(o + slots * 16, 256);
    if (w) w->tab_b = (float*)(base + o);
    o = al3d_align(o + slots * EST_TABB * 4, 256);
    if (w) w->tab_c = (double2*)(base + o);
    o = al3d_align(o + slots * 16, 256);
    return o;
}

static inline int64_t est_weight_elems(int nc)
{
    return (int64_t)EST_C1 * (9 + nc) + EST_C1 + EST_C2 * EST_C1 + EST_C2 + EST_C3 * EST_C2 + EST_C3 +
           EST_C3 * EST_H1 + EST_H1 + EST_H1 * EST_H2 + EST_H2 + EST_H2 + 1;
}

__device__ __forceinline__ float est_lane(float v, int k)
{
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), k));
}

// ---------------------------------------------------------------------------------------------------------- prep
__global__ __launch_bounds__(64) void est_prep_kernel(
    const float* __restrict__ boxes, const int* __restrict__ labels, const int* __restrict__ counts, int nt, int post,
    int box_dim, int rot_col, const int64_t* __restrict__ point_off, int64_t P, int nc, int* __restrict__ nbox,
    float4* __restrict__ tab_a, float* __restrict__ tab_b, double2* __restrict__ tab_c, int* __restrict__ status)
{
    const int b = blockIdx.x, lane = threadIdx.x;
    const int nb = nt * post;
    int bad = 0;
    const int64_t p0 = point_off[b], p1 = point_off[b + 1];
    if (p0 < 0 || p1 < p0 || p1 > P) bad |= AL3D_EST_BAD_OFFSETS;
    int n = 0;
    for (int t = 0; t < nt; ++t) {
        const int cnt = min(max(counts[b * nt + t], 0), post);
        for (int base = 0; base < cnt; base += 64) {
            const int i = base + lane;
            const bool keep = i < cnt;
            const unsigned long long m = __ballot(keep);
            const int j = n + __popcll(m & ((1ull << lane) - 1ull));
            n += __popcll(m);
            if (!keep) continue;
            const int slot = t * post + i;
            const int64_t o = (int64_t)b * nb + slot;
            const int lab = labels[o];
            if (lab < 0 || lab >= nc) bad |= AL3D_EST_BAD_LABEL;
            const float* bx = boxes + o * box_dim;
            const float x = bx[0], y = bx[1], z = bx[2], w = bx[3], l = bx[4], h = bx[5], r = bx[rot_col];
            // sin / cos correctly rounded from double; the double pair itself goes to the feature pass
            const double sd = sin((double)r), cd = cos((double)r);
            const float s = (float)sd, c = (float)cd;
            // center_to_corner_box2d(xy, (w, l) * 2, r): dims * corners_norm, corners_norm = (-.5,-.5) (-.5,.5) (.5,.5) (.5,-.5)
            const float dw = w * 2.0f, dl = l * 2.0f;
            const float lx[4] = {dw * -0.5f, dw * -0.5f, dw * 0.5f, dw * 0.5f};
            const float ly[4] = {dl * -0.5f, dl * 0.5f, dl * 0.5f, dl * -0.5f};
            float cx[4], cy[4];
            for (int k = 0; k < 4; ++k) {
                // rotation_2d: [x y] @ [[cos, -sin], [sin, cos]] -- clockwise for a positive angle -- then + centre
                cx[k] = (lx[k] * c + ly[k] * s) + x;
                cy[k] = (lx[k] * -s + ly[k] * c) + y;
            }
            float* tb = tab_b + ((int64_t)b * nb + j) * EST_TABB;
            for (int k = 0; k < 4; ++k) {
                const int q = (k + 3) & 3;                  // polygon_next = the previous corner (geometry.py:18-21)
                tb[2 * k] = cx[k];
                tb[2 * k + 1] = cy[k];
                tb[8 + 2 * k] = cx[k] - cx[q];
                tb[8 + 2 * k + 1] = cy[k] - cy[q];
            }
            tb[16] = z;
            tb[17] = h / 2.0f;
            tab_c[(int64_t)b * nb + j] = make_double2(sd, cd);
            // every point inside the doubled footprint lies within sqrt(w^2 + l^2) of the centre; 1e-3 relative + 1e-6 covers
            // the rounding of both sides by orders of magnitude.  A NaN box gives a NaN radius: no candidate, as no cross
            // product of the reference's is > 0 then
            const float r2 = (w * w + l * l) * 1.001f + 1e-6f;
            tab_a[(int64_t)b * nb + j] = make_float4(x, y, r2, __int_as_float(slot));
        }
    }
    if (lane == 0) nbox[b] = n;
    if (bad) atomicOr(status, bad);
}

// ---------------------------------------------------------------------------------------------------------- points
__global__ __launch_bounds__(64 * EST_WAVES) void est_points_kernel(
    const float* __restrict__ boxes, const int* __restrict__ labels, int B, int nt, int post, int box_dim,
    const float* __restrict__ points, const int64_t* __restrict__ point_off, int F, const float* __restrict__ wts, int nc,
    const int* __restrict__ nbox, const float4* __restrict__ tab_a, const float* __restrict__ tab_b,
    const double2* __restrict__ tab_c, int* __restrict__ npts, unsigned* __restrict__ pooled, const int* __restrict__ status)
{
    __shared__ unsigned s_queue[EST_WAVES][EST_QCAP];
    if (*status != 0) return;                               // bad offsets or labels: nothing is read or written
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // this wave's (frame, tile): frames own cdiv(points, EST_WTILE) consecutive wave tiles each
    const int64_t wid = (int64_t)blockIdx.x * EST_WAVES + wave;
    int b = -1;
    int64_t tile0 = 0, fp0 = 0, fp1 = 0;
    {
        int64_t acc = 0;
        for (int f = 0; f < B; ++f) {
            const int64_t a = point_off[f], e = point_off[f + 1];
            const int64_t t = (e - a + EST_WTILE - 1) / EST_WTILE;
            if (wid < acc + t) { b = f; tile0 = a + (wid - acc) * EST_WTILE; fp0 = a; fp1 = e; break; }
            acc += t;
        }
    }
    if (b < 0) return;
    (void)fp0;
    const int nb = nt * post;
    const int n = nbox[b];
    if (n == 0) return;
    const float4* ta = tab_a + (int64_t)b * nb;
    const float* tbb = tab_b + (int64_t)b * nb * EST_TABB;
    const double2* tcc = tab_c + (int64_t)b * nb;
    const int nf = 9 + nc;

    float px[EST_PPL], py[EST_PPL], pz[EST_PPL];
    bool live[EST_PPL];
#pragma unroll
    for (int i = 0; i < EST_PPL; ++i) {
        const int64_t g = tile0 + i * 64 + lane;
        live[i] = g < fp1;
        const float* p = points + (live[i] ? g : tile0) * F;
        px[i] = p[0]; py[i] = p[1]; pz[i] = p[2];
    }

    // lane o's rows of the folded point network, loaded at the wave's first drain
    // in double: every product of two f32 values is exact there and a dot product rounds once, at its end.  With f32
    // accumulators the pooled rows of the golden fixture sat 2.1e-7 from float64, the reference's own f32 run 1.3e-7
    // (the weights stay f32 in registers and are widened at use: as doubles they would not fit)
    float w1[9], w2[EST_C1], w3a[EST_C2], w3b[EST_C2], bias1 = 0.f, bias2 = 0.f, bias3a = 0.f, bias3b = 0.f;
    bool loaded = false;
    const float* W1 = wts;
    const float* B1 = W1 + EST_C1 * nf;
    const float* W2 = B1 + EST_C1;
    const float* B2 = W2 + EST_C2 * EST_C1;
    const float* W3 = B2 + EST_C2;
    const float* B3 = W3 + EST_C3 * EST_C2;
    unsigned* queue = s_queue[wave];
    int cnt = 0;
    const unsigned long long lt = (1ull << lane) - 1ull;

    auto drain = [&]() {
        __threadfence_block();
        if (!loaded) {
            const int o1 = lane & (EST_C1 - 1);
#pragma unroll
            for (int k = 0; k < 9; ++k) w1[k] = W1[o1 * nf + k];
            bias1 = B1[o1];
#pragma unroll
            for (int k = 0; k < EST_C1; ++k) w2[k] = W2[lane * EST_C1 + k];
            bias2 = B2[lane];
#pragma unroll
            for (int k = 0; k < EST_C2; ++k) { w3a[k] = W3[lane * EST_C2 + k]; w3b[k] = W3[(lane + 64) * EST_C2 + k]; }
            bias3a = B3[lane];
            bias3b = B3[lane + 64];
            loaded = true;
        }
        int cur = -1, run = 0;                              // the slot whose hits are being reduced, and how many
        float m0 = 0.f, m1 = 0.f;
        for (int q = 0; q <= cnt; ++q) {
            int slot = -1;
            unsigned e = 0;
            if (q < cnt) {
                e = queue[q];
                slot = __float_as_int(ta[e & 0xffffu].w);
            }
            if (slot != cur) {
                if (cur >= 0) {
                    unsigned* row = pooled + ((int64_t)b * nb + cur) * EST_C3;
                    const unsigned u0 = __float_as_uint(m0), u1 = __float_as_uint(m1);
                    if (u0 > row[lane]) atomicMax(row + lane, u0);
                    if (u1 > row[lane + 64]) atomicMax(row + lane + 64, u1);
                    if (lane == 0) atomicAdd(npts + (int64_t)b * nb + cur, run);
                }
                cur = slot; run = 0; m0 = 0.f; m1 = 0.f;
            }
            if (q == cnt) break;
            const int j = (int)(e & 0xffffu);
            const float* p = points + (tile0 + (e >> 16)) * F;
            const float* bx = boxes + ((int64_t)b * nb + slot) * box_dim;
            const int lab = labels[(int64_t)b * nb + slot];
            // instance_points - box[:3], then @ rot_mat_T = [[cos, -sin, 0], [sin, cos, 0], [0, 0, 1]] (estimator.py:240-242,
            // 538-548): the OTHER sense of rotation than the footprint's; both are the reference's.  The nine values are
            // wave-uniform and formed in double, rounded to f32 once: half an ulp each, where the reference's f32 chain
            // (f32 sin / cos times offsets of metres) carries a few 1e-7 m
            const double2 sc = tcc[j];
            const double dx = (double)p[0] - (double)bx[0], dy = (double)p[1] - (double)bx[1];
            const double dz = (double)p[2] - (double)bx[2];
            const double lx = dx * sc.y + dy * sc.x, ly = dy * sc.y - dx * sc.x;
            const double hw = (double)bx[3] * 0.5, hl = (double)bx[4] * 0.5, hh = (double)bx[5] * 0.5;
            const double f[9] = {lx, ly, dz, hw + lx, hw - lx, hl + ly, hl - ly, hh + dz, hh - dz};
            // layer 1 on lanes 0..31 (the upper half repeats it), the one-hot column from memory
            double a = bias1;
#pragma unroll
            for (int k = 0; k < 9; ++k) a = fma(f[k], (double)w1[k], a);
            a += (double)W1[(lane & (EST_C1 - 1)) * nf + 9 + lab];
            const float h1 = a > 0. ? (float)a : 0.f;
            double a2 = bias2, a2b = 0.;
#pragma unroll
            for (int k = 0; k < EST_C1; k += 2) {
                a2 = fma((double)est_lane(h1, k), (double)w2[k], a2);
                a2b = fma((double)est_lane(h1, k + 1), (double)w2[k + 1], a2b);
            }
            a2 += a2b;
            const float h2 = a2 > 0. ? (float)a2 : 0.f;
            double d0 = bias3a, d1 = 0., e0 = bias3b, e1 = 0.;
#pragma unroll
            for (int k = 0; k < EST_C2; k += 2) {
                const double x0 = (double)est_lane(h2, k), x1 = (double)est_lane(h2, k + 1);
                d0 = fma(x0, (double)w3a[k], d0);
                d1 = fma(x1, (double)w3a[k + 1], d1);
                e0 = fma(x0, (double)w3b[k], e0);
                e1 = fma(x1, (double)w3b[k + 1], e1);
            }
            const float u0 = (float)(d0 + d1), v0 = (float)(e0 + e1);
            if (u0 > m0) m0 = u0;
            if (v0 > m1) m1 = v0;
            ++run;
        }
        cnt = 0;
        __threadfence_block();
    };

    float4 next = ta[0];
    for (int j = 0; j < n; ++j) {
        const float4 A = next;                              // wave-uniform: centre x, y, reject radius^2, slot
        next = ta[min(j + 1, n - 1)];                       // the next record's scalar load flies during this box's tests
        bool cand[EST_PPL], any = false;
#pragma unroll
        for (int i = 0; i < EST_PPL; ++i) {
            const float dx = px[i] - A.x, dy = py[i] - A.y;
            cand[i] = live[i] && (dx * dx + dy * dy <= A.z);
            any = any || cand[i];
        }
        if (__ballot(any) == 0ull) continue;
        const float* tb = tbb + (int64_t)j * EST_TABB;
#pragma unroll
        for (int i = 0; i < EST_PPL; ++i) {
            bool hit = cand[i];
            if (hit) {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    // vec1 = corner - previous corner; vec2 = corner - point, flipped, second component negated
                    const float vx = tb[2 * k] - px[i], vy = tb[2 * k + 1] - py[i];
                    const float cross = tb[8 + 2 * k] * vy + tb[8 + 2 * k + 1] * -vx;
                    hit = hit && (cross > 0.f);
                }
                hit = hit && (fabsf(pz[i] - tb[16]) <= tb[17]);
            }
            const unsigned long long m = __ballot(hit);
            if (m) {
                if (hit) queue[cnt + __popcll(m & lt)] = ((unsigned)(i * 64 + lane) << 16) | (unsigned)j;
                cnt += __popcll(m);
            }
        }
        if (cnt > EST_QCAP - EST_WTILE) drain();
    }
    if (cnt > 0) drain();
}

// ---------------------------------------------------------------------------------------------------------- head
__global__ __launch_bounds__(64 * EST_WAVES) void est_head_kernel(
    const float* __restrict__ boxes, const int* __restrict__ labels, const int* __restrict__ counts, int nt, int post,
    int box_dim, const float* __restrict__ wts, int nc, const int* __restrict__ npts, const unsigned* __restrict__ pooled,
    float* __restrict__ out_boxes, float* __restrict__ out_scores, int* __restrict__ out_labels,
    int* __restrict__ out_counts, const int* __restrict__ status)
{
    __shared__ int s_list[AL3D_EST_MAX_BOXES];
    __shared__ int s_n;
    __shared__ float s_x[EST_WAVES][EST_GROUP][EST_C3];
    __shared__ float s_h[EST_WAVES][EST_GROUP][EST_H1];
    if (*status != 0) return;
    const int bt = blockIdx.x;                              // b * nt + t
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t base = (int64_t)bt * post;
    if (wave == 0) {
        const int cnt = min(max(counts[bt], 0), post);
        int n = 0;
        for (int i0 = 0; i0 < cnt; i0 += 64) {
            const int i = i0 + lane;
            const bool keep = i < cnt && npts[base + i] > 0;
            const unsigned long long m = __ballot(keep);
            if (keep) s_list[n + __popcll(m & ((1ull << lane) - 1ull))] = i;
            n += __popcll(m);
        }
        if (lane == 0) { s_n = n; out_counts[bt] = n; }
    }
    __syncthreads();
    const int n = s_n;
    const float* H1 = wts + EST_C1 * (9 + nc) + EST_C1 + EST_C2 * EST_C1 + EST_C2 + EST_C3 * EST_C2 + EST_C3;   // [128][256]
    const float* C1 = H1 + EST_C3 * EST_H1;
    const float* H2 = C1 + EST_H1;                                                                              // [256][64]
    const float* C2 = H2 + EST_H1 * EST_H2;
    const float* H3 = C2 + EST_H2;
    const float* C3 = H3 + EST_H2;
    for (int g0 = wave * EST_GROUP; g0 < n; g0 += EST_WAVES * EST_GROUP) {
        const int ng = min(EST_GROUP, n - g0);
        for (int g = 0; g < EST_GROUP; ++g) {
            const unsigned* row = pooled + (base + s_list[g0 + min(g, ng - 1)]) * EST_C3;
            s_x[wave][g][lane] = __uint_as_float(row[lane]);
            s_x[wave][g][lane + 64] = __uint_as_float(row[lane + 64]);
        }
        __threadfence_block();
        // in double, as the point network: sequential f32 fmaf chains of 128 and 256 terms left the score one f32 ulp
        // from the correctly rounded one on some boxes (4.9e-8 from float64 where a float32 torch evaluation is at 1.1e-8)
        double acc[4][EST_GROUP];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int g = 0; g < EST_GROUP; ++g) acc[i][g] = (double)C1[lane + 64 * i];
        for (int k = 0; k < EST_C3; ++k) {
            double w[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) w[i] = (double)H1[k * EST_H1 + lane + 64 * i];
#pragma unroll
            for (int g = 0; g < EST_GROUP; ++g) {
                const double x = (double)s_x[wave][g][k];
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[i][g] = fma(x, w[i], acc[i][g]);
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int g = 0; g < EST_GROUP; ++g) s_h[wave][g][lane + 64 * i] = acc[i][g] > 0. ? (float)acc[i][g] : 0.f;
        __threadfence_block();
        double a2[EST_GROUP];
#pragma unroll
        for (int g = 0; g < EST_GROUP; ++g) a2[g] = (double)C2[lane];
        for (int k = 0; k < EST_H1; ++k) {
            const double w = (double)H2[k * EST_H2 + lane];
#pragma unroll
            for (int g = 0; g < EST_GROUP; ++g) a2[g] = fma((double)s_h[wave][g][k], w, a2[g]);
        }
        const double w3 = (double)H3[lane];
#pragma unroll
        for (int g = 0; g < EST_GROUP; ++g) {
            double v = (a2[g] > 0. ? (double)(float)a2[g] : 0.) * w3;
            for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
            if (g < ng) {
                const int src = s_list[g0 + g], dst = g0 + g;
                if (lane == 0) {
                    out_scores[base + dst] = (float)(1.0 / (1.0 + exp(-(v + (double)C3[0]))));
                    out_labels[base + dst] = labels[base + src];
                }
                if (lane < box_dim) out_boxes[(base + dst) * box_dim + lane] = boxes[(base + src) * box_dim + lane];
            }
        }
        __threadfence_block();
    }
}

extern "C" int64_t al3d_estimator_workspace_bytes(int B, int nt, int post)
{
    if (B < 0 || nt < 1 || post < 1 || (int64_t)nt * post > AL3D_EST_MAX_BOXES) return -1;
    return est_ws_layout(B, nt, post, nullptr, nullptr) + 256;
}

extern "C" int64_t al3d_estimator_weight_elems(int num_classes)
{
    if (num_classes < 1 || num_classes > AL3D_EST_MAX_CLASSES) return -1;
    return est_weight_elems(num_classes);
}

extern "C" int al3d_estimator_f32(const float* boxes, const int* labels, const int* counts, int B, int nt, int post,
                                  int box_dim, int rot_col, const float* points, const int64_t* point_off, int64_t P, int F,
                                  const float* wts, int64_t wts_elems, int num_classes, float* out_boxes, float* out_scores,
                                  int* out_labels, int* out_counts, void* workspace, int* status, void* stream)
{
    AL3D_REQUIRE(B >= 0 && nt >= 1 && post >= 1 && P >= 0 && F >= 3, "al3d_estimator_f32: bad sizes");
    AL3D_REQUIRE(box_dim >= 6 && box_dim <= 64 && rot_col >= 0 && rot_col < box_dim, "al3d_estimator_f32: bad box layout");
    AL3D_REQUIRE((int64_t)nt * post <= AL3D_EST_MAX_BOXES,
                 "al3d_estimator_f32: nt * post = %lld boxes per frame, at most %d", (long long)nt * post, AL3D_EST_MAX_BOXES);
    AL3D_REQUIRE(num_classes >= 1 && num_classes <= AL3D_EST_MAX_CLASSES,
                 "al3d_estimator_f32: num_classes %d outside [1, %d]", num_classes, AL3D_EST_MAX_CLASSES);
    AL3D_REQUIRE(wts_elems == est_weight_elems(num_classes), "al3d_estimator_f32: packed weights hold %lld floats, %lld expected",
                 (long long)wts_elems, (long long)est_weight_elems(num_classes));
    AL3D_REQUIRE((int64_t)B * nt * post < (1LL << 31) / 64 && B < (1 << 20) && P < (1LL << 40),
                 "al3d_estimator_f32: batch too large");
    AL3D_REQUIRE(status, "al3d_estimator_f32: null pointer");
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(status, 0, sizeof(int), st) != hipSuccess) return al3d_fail(AL3D_ELAUNCH, "al3d_estimator_f32: memset");
    if (B == 0) return AL3D_OK;
    AL3D_REQUIRE(boxes && labels && counts && point_off && wts && out_boxes && out_scores && out_labels && out_counts &&
                 workspace, "al3d_estimator_f32: null pointer");
    AL3D_REQUIRE(P == 0 || points, "al3d_estimator_f32: null pointer");
    EstWs w;
    char* base = (char*)(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
    est_ws_layout(B, nt, post, base, &w);
    const size_t slots = (size_t)B * nt * post;
    if (hipMemsetAsync(w.npts, 0, slots * sizeof(int), st) != hipSuccess ||
        hipMemsetAsync(w.pooled, 0, slots * EST_C3 * sizeof(unsigned), st) != hipSuccess)
        return al3d_fail(AL3D_ELAUNCH, "al3d_estimator_f32: memset");
    hipLaunchKernelGGL(est_prep_kernel, dim3((unsigned)B), dim3(64), 0, st, boxes, labels, counts, nt, post, box_dim, rot_col,
                       point_off, P, num_classes, w.nbox, w.tab_a, w.tab_b, w.tab_c, status);
    AL3D_CHECK_LAUNCH("est_prep_kernel");
    // sum over frames of cdiv(points, tile) <= cdiv(P, tile) + B wave tiles
    const int64_t waves = al3d_cdiv(P, EST_WTILE) + B;
    if (P > 0) {
        hipLaunchKernelGGL(est_points_kernel, dim3((unsigned)al3d_cdiv(waves, EST_WAVES)), dim3(64 * EST_WAVES), 0, st, boxes,
                           labels, B, nt, post, box_dim, points, point_off, F, wts, num_classes, w.nbox, w.tab_a, w.tab_b,
                           w.tab_c, w.npts, w.pooled, status);
        AL3D_CHECK_LAUNCH("est_points_kernel");
    }
    hipLaunchKernelGGL(est_head_kernel, dim3((unsigned)(B * nt)), dim3(64 * EST_WAVES), 0, st, boxes, labels, counts, nt, post,
                       box_dim, wts, num_classes, w.npts, w.pooled, out_boxes, out_scores, out_labels, out_counts, status);
    AL3D_CHECK_LAUNCH("est_head_kernel");
    return AL3D_OK;
}
