// Point-in-box membership with a stable per-box compaction: the device half of the ground-truth database builder
// (reference det3d/datasets/utils/create_gt_database.py:101-152 over box_np_ops.points_in_rbbox, box_np_ops.py:1102-1108,
// and geometry.py:243-304 -- the python triple loop over points, boxes and the six planes of a box).
//
// The planes come from the host (detector_ops.box_planes, the reference's own float32 calls); the kernels only apply the
// sign rule of geometry.py:290-303: a point is inside iff, for all six planes, !(sign >= 0) with
// sign = ((x*n0 + y*n1) + z*n2) + d, every product and sum rounded to float32 (no contraction: __fmul_rn / __fadd_rn, and
// the file is built with -ffp-contract=off).  A NaN sign counts as inside; a zero-size box (n = d = 0) holds nothing.
//
// Shape.  grid = (groups, frames); every WAVE owns one contiguous span of its frame's points (a "slot": slots =
// groups * waves per workgroup, span = a multiple of 64) and walks it 64 points at a time, one lane per point.  The frame's
// planes pass through LDS `tile` boxes at a time (64 boxes = 6 KB, read by broadcast).  A box's members in the wave are a
// ballot; lane j keeps the running count (count pass) or the running output row (gather pass) of the tile's box j.
//   count : part[r, slot] = members of box r in that slot; box_count[r] += it (integer atomics: the sum has no order).
//           The host entry then runs the exclusive scan of csrc/al3d_scan.h over part, flattened.
//   gather: the first output row of (r, slot) is out_off[r] + (scan[r, slot] - scan[r, 0]); inside the wave a member's row
//           adds the popcount of the lower lanes.  Slots are ascending point ranges, so every box's rows are in ascending
//           point index whatever the launch shape.  No float atomics, no dependence on the order of execution.
#include "al3d_common.h"
#include "al3d_scan.h"

#define PIB_TILE 64                 // boxes in LDS at a time
#define PIB_HDR_BYTES 256           // workspace header: int[0] = magic, [1] = slots, [2] = R, [3] = B
#define PIB_MAGIC 0x50494231        // "PIB1"

// geometry.py:290-303 on one box: six planes (n0, n1, n2, d) in LDS
__device__ __forceinline__ bool pib_inside(const float4* __restrict__ pl, float x, float y, float z)
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

// a frame's points [p0, p0 + n) and boxes [r0, r0 + nb); bad offsets -> an empty frame and the status bits
__device__ __forceinline__ int pib_frame(const int64_t* __restrict__ point_off, const int* __restrict__ box_off, int b,
                                         int64_t P, int R, int64_t& p0, int64_t& n, int& r0, int& nb)
{
    int bad = 0;
    const int64_t q0 = point_off[b], q1 = point_off[b + 1];
    const int s0 = box_off[b], s1 = box_off[b + 1];
    if (q0 < 0 || q1 < q0 || q1 > P) bad |= AL3D_PIB_BAD_POINT_OFF;
    else if (q1 - q0 >= (1LL << 31)) bad |= AL3D_PIB_FRAME_TOO_LARGE;
    if (s0 < 0 || s1 < s0 || s1 > R) bad |= AL3D_PIB_BAD_BOX_OFF;
    p0 = bad ? 0 : q0;
    n = bad ? 0 : q1 - q0;
    r0 = bad ? 0 : s0;
    nb = bad ? 0 : s1 - s0;
    return bad;
}

__device__ __forceinline__ int64_t pib_shfl64(int64_t v, int src)
{
    const int lo = __shfl((int)(v & 0xffffffffLL), src);
    const int hi = __shfl((int)(v >> 32), src);
    return ((int64_t)hi << 32) | (uint32_t)lo;
}

template <bool GATHER>
__global__ __launch_bounds__(256) void pib_walk_kernel(
    const float* __restrict__ points, int64_t P, int F, const int64_t* __restrict__ point_off,
    const float* __restrict__ planes, const int* __restrict__ box_off, int R, int tile, int* __restrict__ hdr,
    int* __restrict__ part, int* __restrict__ box_count, const int64_t* __restrict__ out_off,
    const float* __restrict__ centres, float* __restrict__ out, int F_out, int64_t* __restrict__ out_index, int64_t T,
    int* __restrict__ status)
{
    __shared__ float4 s_pl[PIB_TILE * 6];
    __shared__ float s_ctr[PIB_TILE * 3];

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, W = blockDim.x >> 6;
    const int b = blockIdx.y;
    const int S = gridDim.x * W, slot = blockIdx.x * W + wave;

    if (GATHER) {
        // the partial counts were written for one number of slots: refuse a workspace of another launch shape
        if (hdr[0] != PIB_MAGIC || hdr[1] != S || hdr[2] != R || hdr[3] != (int)gridDim.y) {
            if (threadIdx.x == 0) atomicOr(status, AL3D_PIB_BAD_WORKSPACE);
            return;
        }
    } else if (blockIdx.x == 0 && b == 0 && threadIdx.x == 0) {
        hdr[0] = PIB_MAGIC; hdr[1] = S; hdr[2] = R; hdr[3] = (int)gridDim.y;
    }

    int64_t p0, n;
    int r0, nb;
    int bad = pib_frame(point_off, box_off, b, P, R, p0, n, r0, nb);

    // this wave's span of the frame: a multiple of 64 points, so every wave but a span's last one is full
    const int64_t per = ((n + S - 1) / S + 63) / 64 * 64;
    const int64_t start = min(n, (int64_t)slot * per), end = min(n, start + per);

    for (int t0 = 0; t0 < nb; t0 += tile) {
        const int tb = min(tile, nb - t0);
        __syncthreads();                                   // the previous tile has been read by every wave
        for (int i = threadIdx.x; i < tb * 6; i += blockDim.x)
            s_pl[i] = reinterpret_cast<const float4*>(planes)[(int64_t)(r0 + t0) * 6 + i];
        if (GATHER)
            for (int i = threadIdx.x; i < tb * 3; i += blockDim.x) s_ctr[i] = centres[(int64_t)(r0 + t0) * 3 + i];
        __syncthreads();

        // lane j: box t0 + j of the frame
        const int64_t rj = (int64_t)(r0 + t0 + lane) * S;  // its row of part (read only for lane < tb)
        int acc = 0;
        int64_t base = 0;
        if (GATHER && lane < tb)
            base = out_off[r0 + t0 + lane] + (int64_t)((unsigned)part[rj + slot] - (unsigned)part[rj]);

        for (int64_t i0 = start; i0 < end; i0 += 64) {
            const int64_t i = i0 + lane;
            const bool live = i < end;
            const float* p = points + (p0 + (live ? i : start)) * F;
            const float x = p[0], y = p[1], z = p[2];
            for (int j = 0; j < tb; ++j) {
                const bool in = live && pib_inside(&s_pl[j * 6], x, y, z);
                const unsigned long long m = __ballot(in);
                if (m == 0ull) continue;                   // wave-uniform
                const int cnt = __popcll(m);
                if (GATHER) {
                    const int64_t bj = pib_shfl64(base, j);
                    if (in) {
                        const int64_t row = bj + __popcll(m & ((1ull << lane) - 1ull));
                        if (row >= 0 && row < T) {
                            float* o = out + row * F_out;
                            o[0] = __fsub_rn(x, s_ctr[j * 3]);
                            o[1] = __fsub_rn(y, s_ctr[j * 3 + 1]);
                            o[2] = __fsub_rn(z, s_ctr[j * 3 + 2]);
                            for (int c = 3; c < F_out; ++c) o[c] = p[c];
                            out_index[row] = p0 + i;
                        } else {
                            bad |= AL3D_PIB_BAD_ROWS;
                        }
                    }
                    if (lane == j) base += cnt;
                } else {
                    if (lane == j) acc += cnt;
                }
            }
        }
        if (!GATHER && lane < tb) {
            part[rj + slot] = acc;
            if (acc) atomicAdd(&box_count[r0 + t0 + lane], acc);
        }
    }
    if (bad) atomicOr(status, bad);
}

// The points_in_rbbox matrix of one frame: out[i, j] = point i inside box j (box_np_ops.py:1102-1108).
__global__ __launch_bounds__(256) void pib_mask_kernel(const float* __restrict__ points, int64_t P, int F,
                                                       const float* __restrict__ planes, int R, int tile,
                                                       unsigned char* __restrict__ out)
{
    __shared__ float4 s_pl[PIB_TILE * 6];
    for (int t0 = 0; t0 < R; t0 += tile) {
        const int tb = min(tile, R - t0);
        __syncthreads();
        for (int i = threadIdx.x; i < tb * 6; i += blockDim.x)
            s_pl[i] = reinterpret_cast<const float4*>(planes)[(int64_t)t0 * 6 + i];
        __syncthreads();
        for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < P; i += (int64_t)gridDim.x * blockDim.x) {
            const float* p = points + i * F;
            const float x = p[0], y = p[1], z = p[2];
            unsigned char* o = out + i * R + t0;
            for (int j = 0; j < tb; ++j) o[j] = pib_inside(&s_pl[j * 6], x, y, z) ? 1 : 0;
        }
    }
}

static bool pib_shape_ok(int groups, int threads, int tile)
{
    return groups >= 1 && groups <= 1024 && (threads == 64 || threads == 128 || threads == 256) && tile >= 1 &&
           tile <= PIB_TILE;
}

static int64_t pib_part_bytes(int64_t R, int64_t slots) { return al3d_align(R * slots * 4, 256); }

extern "C" int64_t al3d_points_in_boxes_workspace_bytes(int64_t R, int groups, int threads)
{
    if (R < 0 || R >= (1LL << 31) || !pib_shape_ok(groups, threads, 1)) return -1;
    const int64_t slots = (int64_t)groups * (threads / 64);
    return PIB_HDR_BYTES + pib_part_bytes(R, slots) + al3d_scan_workspace_bytes(R * slots);
}

static int pib_check(const char* who, const float* points, int64_t P, int F, const int64_t* point_off, int B,
                     const float* planes, const int* box_off, int R, const int* status, int groups, int threads, int tile)
{
    AL3D_REQUIRE(P >= 0 && F >= 3 && B >= 0 && B < 65536 && R >= 0, "%s: bad sizes", who);
    AL3D_REQUIRE(pib_shape_ok(groups, threads, tile), "%s: groups in [1, 1024], threads 64 / 128 / 256, tile in [1, 64]", who);
    AL3D_REQUIRE(status, "%s: null pointer", who);
    if (B == 0) return AL3D_OK;
    AL3D_REQUIRE(point_off && box_off, "%s: null pointer", who);
    AL3D_REQUIRE(P == 0 || points, "%s: null pointer", who);
    AL3D_REQUIRE(R == 0 || planes, "%s: null pointer", who);
    return AL3D_OK;
}

extern "C" int al3d_points_in_boxes_count_launch_f32(const float* points, int64_t P, int F, const int64_t* point_off, int B,
                                                     const float* planes, const int* box_off, int R, int* box_count,
                                                     void* workspace, int* status, int groups, int threads, int tile,
                                                     void* stream)
{
    const char* who = "al3d_points_in_boxes_count_f32";
    const int rc = pib_check(who, points, P, F, point_off, B, planes, box_off, R, status, groups, threads, tile);
    if (rc != AL3D_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(status, 0, sizeof(int), st) != hipSuccess) return al3d_fail(AL3D_ELAUNCH, "%s: memset", who);
    if (R == 0) return AL3D_OK;
    AL3D_REQUIRE(box_count, "%s: null pointer", who);
    if (hipMemsetAsync(box_count, 0, (size_t)R * sizeof(int), st) != hipSuccess)
        return al3d_fail(AL3D_ELAUNCH, "%s: memset", who);
    if (B == 0) return AL3D_OK;
    AL3D_REQUIRE(workspace, "%s: null pointer", who);
    const int64_t slots = (int64_t)groups * (threads / 64);
    int* hdr = (int*)workspace;
    int* part = (int*)((char*)workspace + PIB_HDR_BYTES);
    void* scan_ws = (char*)workspace + PIB_HDR_BYTES + pib_part_bytes(R, slots);
    // a frame with bad offsets writes no partial counts: zero them, the scan reads every one
    if (hipMemsetAsync(part, 0, (size_t)pib_part_bytes(R, slots), st) != hipSuccess)
        return al3d_fail(AL3D_ELAUNCH, "%s: memset", who);
    hipLaunchKernelGGL(pib_walk_kernel<false>, dim3((unsigned)groups, (unsigned)B), dim3((unsigned)threads), 0, st, points, P,
                       F, point_off, planes, box_off, R, tile, hdr, part, box_count, (const int64_t*)nullptr,
                       (const float*)nullptr, (float*)nullptr, 0, (int64_t*)nullptr, (int64_t)0, status);
    AL3D_CHECK_LAUNCH("pib_walk_kernel<count>");
    return al3d_exclusive_scan_i32(part, part, R * slots, scan_ws, st);
}

extern "C" int al3d_points_in_boxes_count_f32(const float* points, int64_t P, int F, const int64_t* point_off, int B,
                                              const float* planes, const int* box_off, int R, int* box_count,
                                              void* workspace, int* status, void* stream)
{
    return al3d_points_in_boxes_count_launch_f32(points, P, F, point_off, B, planes, box_off, R, box_count, workspace, status,
                                                 AL3D_PIB_GROUPS, AL3D_PIB_THREADS, PIB_TILE, stream);
}

extern "C" int al3d_points_in_boxes_gather_launch_f32(const float* points, int64_t P, int F, const int64_t* point_off, int B,
                                                      const float* planes, const int* box_off, int R, const int64_t* out_off,
                                                      const float* centres, const void* workspace, float* out, int F_out,
                                                      int64_t* out_index, int64_t T, int* status, int groups, int threads,
                                                      int tile, void* stream)
{
    const char* who = "al3d_points_in_boxes_gather_f32";
    const int rc = pib_check(who, points, P, F, point_off, B, planes, box_off, R, status, groups, threads, tile);
    if (rc != AL3D_OK) return rc;
    AL3D_REQUIRE(F_out >= 3 && F_out <= F && T >= 0, "%s: need 3 <= F_out <= F and T >= 0", who);
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(status, 0, sizeof(int), st) != hipSuccess) return al3d_fail(AL3D_ELAUNCH, "%s: memset", who);
    if (R == 0 || B == 0) return AL3D_OK;
    AL3D_REQUIRE(out_off && centres && workspace, "%s: null pointer", who);
    AL3D_REQUIRE(T == 0 || (out && out_index), "%s: null pointer", who);
    const int* hdr = (const int*)workspace;
    const int* part = (const int*)((const char*)workspace + PIB_HDR_BYTES);
    hipLaunchKernelGGL(pib_walk_kernel<true>, dim3((unsigned)groups, (unsigned)B), dim3((unsigned)threads), 0, st, points, P,
                       F, point_off, planes, box_off, R, tile, const_cast<int*>(hdr), const_cast<int*>(part), (int*)nullptr,
                       out_off, centres, out, F_out, out_index, T, status);
    AL3D_CHECK_LAUNCH("pib_walk_kernel<gather>");
    return AL3D_OK;
}

extern "C" int al3d_points_in_boxes_gather_f32(const float* points, int64_t P, int F, const int64_t* point_off, int B,
                                               const float* planes, const int* box_off, int R, const int64_t* out_off,
                                               const float* centres, const void* workspace, float* out, int F_out,
                                               int64_t* out_index, int64_t T, int* status, void* stream)
{
    return al3d_points_in_boxes_gather_launch_f32(points, P, F, point_off, B, planes, box_off, R, out_off, centres, workspace,
                                                  out, F_out, out_index, T, status, AL3D_PIB_GROUPS, AL3D_PIB_THREADS,
                                                  PIB_TILE, stream);
}

extern "C" int al3d_points_in_boxes_mask_launch_u8(const float* points, int64_t P, int F, const float* planes, int R,
                                                   unsigned char* out, int threads, int tile, void* stream)
{
    const char* who = "al3d_points_in_boxes_mask_u8";
    AL3D_REQUIRE(P >= 0 && F >= 3 && R >= 0, "%s: bad sizes", who);
    AL3D_REQUIRE(pib_shape_ok(1, threads, tile), "%s: threads 64 / 128 / 256, tile in [1, 64]", who);
    if (P == 0 || R == 0) return AL3D_OK;
    AL3D_REQUIRE(points && planes && out, "%s: null pointer", who);
    const int64_t blocks = al3d_cdiv(P, threads);
    hipLaunchKernelGGL(pib_mask_kernel, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3((unsigned)threads), 0,
                       (hipStream_t)stream, points, P, F, planes, R, tile, out);
    AL3D_CHECK_LAUNCH("pib_mask_kernel");
    return AL3D_OK;
}

extern "C" int al3d_points_in_boxes_mask_u8(const float* points, int64_t P, int F, const float* planes, int R,
                                            unsigned char* out, void* stream)
{
    return al3d_points_in_boxes_mask_launch_u8(points, P, F, planes, R, out, AL3D_PIB_THREADS, PIB_TILE, stream);
}
