// Dynamic voxelisation (no per-voxel or per-frame cap) + scatter reduction for a batch of frames, deterministic.
//
// Reference semantics (bevfusion/mmdet3d/ops/voxel/src/voxelization_cuda.cu:19-60 dynamic_voxelize_kernel,
// src/scatter_points_cuda.cu:183-239 dynamic_point_to_voxel_forward_gpu, ops/voxel/scatter_points.py:85-94):
//   c = floor((p_xyz - range_min) / voxel_size) in float32; a point is kept iff 0 <= c < grid on all three axes, a dropped
//   point has the coordinates (-1, -1, -1); the voxels of a frame are the distinct kept cells in ascending lexicographic
//   order of the coordinate triple (at::unique_dim, sorted, after the -1 row is removed); every point of a voxel takes part
//   in the reduction (sum / mean / max).
// Where this file decides something the reference leaves open:
//   * a NaN coordinate is dropped, as the hard voxelizer does (the reference's `int c = floor(NaN)` is undefined);
//   * the reference sums with atomicAdd in whatever order the points arrive; here the float32 sum starts at 0.f and adds
//     the points in ascending point index -- one of the reference's legal orders, and the order of the hard voxelizer's
//     vox_gather_fixed_kernel, so the two voxelizers give the same bits wherever no cap bites.  mean = sum / (float)count;
//   * max orders floats by their bit pattern (-0.f < +0.f), so it does not depend on the point order; NaN features are
//     outside its contract.
// There is no grid of 4 bytes per cell.  The kept cells are ONE presence bit per cell per frame; the number of set bits
// below a cell's bit is the voxel's row, so the sorted order costs no sort:
//   (1) per point: key (the cell id in the requested order) and one atomicOr per run of equal adjacent lanes,
//   (2) popcount per 128-bit group + exclusive scan = rows before each group (and the per-frame row bases),
//   (3) per point: row = group base + popcount below the bit; one integer atomicAdd per run counts the voxel's points and
//       hands out bucket slots; the run's first lane writes the voxel's coordinates,
//   (4) scan of the counts, bucket the point indices,
//   (5) per voxel: order the bucket by ascending point index and accumulate in that order.  A voxel of at most VD_REG
//       points takes one lane (a sorted register array); one of at most VD_LIGHT points takes a wave: every lane ranks
//       its index among the voxel's by shuffles, a permute puts the indices in order, the adds read the lanes in turn;
//       a heavier one takes a workgroup: every thread ranks indices among the voxel's, the features are staged through
//       LDS in that order, one lane per feature adds.
// The only atomics are integer (or / add) and their return values decide bucket slots alone, which step (5) re-orders:
// every output is a pure function of the inputs.  Built with -ffp-contract=off.
#include "al3d_common.h"
#include "al3d_scan.h"
#include "vox_cell.h"

#define VD_LIGHT 64
#define VD_REG 8        // voxels of at most this many points take one lane; up to VD_LIGHT (the wave size) one wave
#define VD_HEAVY_THREADS 256
#define VD_STAGE_FLOATS 4096
#define VD_MAX_NFEAT 256
#define VD_ST_OVERFLOW 1
#define VD_ST_BAD_COORD 2

// key = (a0 * d1 + a1) * d2 + a2; an output coordinate row is (b, a0, a1, a2) for ncol = 4 and (a0, a1, a2) for ncol = 3
struct VdDims { int d0, d1, d2, ncol; };

// true for a lane that continues the (frame, key) run of the lane below it; every lane of the wave must call it
__device__ __forceinline__ bool vd_continues_run(int key, int b)
{
    const int lane = threadIdx.x & 63;
    const int k1 = __shfl_up(key, 1), b1 = __shfl_up(b, 1);
    return lane > 0 && key >= 0 && k1 == key && b1 == b;
}

// pass 1a: keys from points
__global__ __launch_bounds__(256) void vd_key_points_kernel(const float* __restrict__ pts, const int64_t* __restrict__ off,
                                                            int B, int64_t npts, VoxCfg c, int order, int64_t fwords,
                                                            unsigned* __restrict__ bits, int* __restrict__ pkey,
                                                            int* __restrict__ pframe, int* __restrict__ point_coords)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    // points past point_offsets[B] belong to no frame
    int64_t nlim = off[B];
    if (nlim > npts) nlim = npts;
    int key = -1, b = 0;
    if (i < npts) {
        int x = -1, y = -1, z = -1;
        if (i < nlim) {
            b = frame_of_wave(off, B, i);
            const float* p = pts + i * c.nfeat;
            const float p3[3] = {p[0], p[1], p[2]};
            const int64_t cell = vox_cell(p3, c);
            if (cell >= 0) {                       // cells < 2^31 is checked on the host
                const int ci = (int)cell;
                x = ci % c.gx; y = (ci / c.gx) % c.gy; z = ci / (c.gx * c.gy);
                key = order == 0 ? ci : (x * c.gy + y) * c.gz + z;
            }
        }
        if (point_coords) { point_coords[3 * i] = x; point_coords[3 * i + 1] = y; point_coords[3 * i + 2] = z; }
        pkey[i] = key;
        pframe[i] = b;
    }
    // a ring scan puts neighbouring returns into the same voxel: one atomic per run of equal adjacent lanes
    const bool same = vd_continues_run(key, b);
    if (key >= 0 && !same) atomicOr(&bits[(int64_t)b * fwords + (key >> 5)], 1u << (key & 31));
}

// pass 1b: keys from given integer coordinates [n,3]; a row with a negative coordinate is dropped
// (scatter_points_cuda.cu:202), one beyond the stated extents is refused through the status word
__global__ __launch_bounds__(256) void vd_key_coors_kernel(const int* __restrict__ coors, int64_t n, VdDims d,
                                                           unsigned* __restrict__ bits, int* __restrict__ pkey,
                                                           int* __restrict__ pframe, int* __restrict__ status)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int key = -1;
    if (i < n) {
        const int a0 = coors[3 * i], a1 = coors[3 * i + 1], a2 = coors[3 * i + 2];
        if (a0 >= 0 && a1 >= 0 && a2 >= 0) {
            if (a0 < d.d0 && a1 < d.d1 && a2 < d.d2) key = (a0 * d.d1 + a1) * d.d2 + a2;
            else atomicOr(status, VD_ST_BAD_COORD);
        }
        pkey[i] = key;
        pframe[i] = 0;
    }
    const bool same = vd_continues_run(key, 0);
    if (key >= 0 && !same) atomicOr(&bits[key >> 5], 1u << (key & 31));
}

// pass 2: set bits per 128-bit group (the scan's input has one more element: its last output is the total)
__global__ __launch_bounds__(256) void vd_popc_kernel(const uint4* __restrict__ bits, int64_t G, int* __restrict__ gcnt)
{
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g > G) return;
    int n = 0;
    if (g < G) {
        const uint4 w = bits[g];
        n = __popc(w.x) + __popc(w.y) + __popc(w.z) + __popc(w.w);
    }
    gcnt[g] = n;
}

// voxels per frame and row bases (frames are concatenated in the outputs); more rows than rows_cap sets the status
__global__ void vd_base_kernel(const int* __restrict__ gscan, int64_t fgroups, int B, int64_t rows_cap,
                               int* __restrict__ num_voxels, int* __restrict__ row_base, int* __restrict__ status)
{
    for (int b = threadIdx.x; b <= B; b += blockDim.x) {
        const int base = gscan[(int64_t)b * fgroups];
        row_base[b] = base;
        if (b < B) num_voxels[b] = gscan[(int64_t)(b + 1) * fgroups] - base;
        else if (base > rows_cap) atomicOr(status, VD_ST_OVERFLOW);
    }
}

// pass 3: row per point (or -1), points per voxel, bucket slot per point, coordinates of the voxels
__global__ __launch_bounds__(256) void vd_assign_kernel(int64_t npts, VdDims d, int64_t fwords,
                                                        const unsigned* __restrict__ bits, const int* __restrict__ gscan,
                                                        const int* __restrict__ pkey, const int* __restrict__ pframe,
                                                        int64_t nrows, int* __restrict__ prow, int* __restrict__ ppos,
                                                        int* __restrict__ cnt, int* __restrict__ coords,
                                                        int* __restrict__ point2voxel)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int key = -1, b = 0;
    if (i < npts) { key = pkey[i]; b = pframe[i]; }
    // runs of adjacent lanes of one voxel: the run's first lane ranks the bit and takes the run's slots with ONE atomicAdd,
    // the others derive theirs (slot order inside a voxel is irrelevant: the reduction orders the bucket)
    const int lane = threadIdx.x & 63;
    const bool same = vd_continues_run(key, b);
    const unsigned long long starts = __ballot(!same);
    const unsigned long long upto = (2ull << lane) - 1ull;
    const int start = 63 - __builtin_clzll(starts & upto);
    const unsigned long long later = starts & ~upto;
    const int end = later ? (int)__builtin_ctzll(later) : 64;
    int row = -1, pos = 0;
    if (key >= 0 && !same) {
        const int w = key >> 5;
        const unsigned* wp = bits + (int64_t)b * fwords;
        int r = gscan[(int64_t)b * (fwords >> 2) + (w >> 2)];
        for (int k = w & ~3; k < w; ++k) r += __popc(wp[k]);
        r += __popc(wp[w] & ((1u << (key & 31)) - 1u));
        if (r < nrows) {                             // nothing is written past rows_cap
            row = r;
            pos = atomicAdd(&cnt[row], end - start);
            const int a2 = key % d.d2, a1 = (key / d.d2) % d.d1, a0 = key / (d.d1 * d.d2);
            if (d.ncol == 4) *reinterpret_cast<int4*>(coords + 4 * (int64_t)row) = make_int4(b, a0, a1, a2);
            else { int* cr = coords + 3 * (int64_t)row; cr[0] = a0; cr[1] = a1; cr[2] = a2; }
        }
    }
    row = __shfl(row, start);
    pos = __shfl(pos, start) + (lane - start);
    if (row < 0) pos = 0;
    if (i < npts) {
        prow[i] = row;
        ppos[i] = pos;
        if (point2voxel) point2voxel[i] = row;
    }
}

// pass 4: bucket the point indices per voxel at the slots pass 3 handed out
__global__ __launch_bounds__(256) void vd_bucket_kernel(int64_t npts, const int* __restrict__ prow,
                                                        const int* __restrict__ ppos, const int* __restrict__ boff,
                                                        int* __restrict__ bucket)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npts) return;
    const int row = prow[i];
    if (row < 0) return;
    bucket[boff[row] + ppos[i]] = (int)i;
}

// floats in the order of their bit patterns: -0.f below +0.f
__device__ __forceinline__ int vd_ord(float f)
{
    const int b = __float_as_int(f);
    return b ^ ((b >> 31) & 0x7fffffff);
}

// one step of the reduction in ascending point order (reduce: 0 sum, 1 mean, 2 max; acc starts at 0.f)
__device__ __forceinline__ float vd_step(float acc, float v, bool first, int reduce)
{
    if (reduce == 2) return (first || vd_ord(v) > vd_ord(acc)) ? v : acc;
    return acc + v;
}

// pass 5a: one lane per voxel of at most VD_REG points; larger voxels are listed for pass 5b (up to VD_LIGHT points) or
// 5c (the lists' order is irrelevant: each entry is reduced on its own).  NF > 0: the feature count, accumulators in
// registers; 0: any count.
template <int NF>
__global__ __launch_bounds__(128) void vd_reduce_kernel(const float* __restrict__ pts, int nfeat, int reduce,
                                                        int64_t nrows, const int* __restrict__ total,
                                                        const int* __restrict__ boff, const int* __restrict__ cnt,
                                                        int* __restrict__ bucket, float* __restrict__ feat,
                                                        int* __restrict__ counts, int* __restrict__ heavy,
                                                        int* __restrict__ nheavy, int* __restrict__ mid,
                                                        int* __restrict__ nmid)
{
    const int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= nrows || row >= *total) return;
    const int n = cnt[row], o = boff[row];
    counts[row] = n;
    if (n > VD_LIGHT) { heavy[atomicAdd(nheavy, 1)] = (int)row; return; }
    if (n > VD_REG) { mid[atomicAdd(nmid, 1)] = (int)row; return; }
    const float denom = (float)n;
    if (NF > 0) {
        // the common case, a handful of points: the indices sit in a sorted register array (compile-time indexed
        // compare-exchange chain, as in the hard voxelizer's gather), so neither the index loads nor the point loads wait
        // for one another; only the adds run in order
        int sel[VD_REG];
#pragma unroll
        for (int i = 0; i < VD_REG; ++i) sel[i] = 0x7fffffff;
#pragma unroll
        for (int t = 0; t < VD_REG; ++t) {
            int idx = t < n ? bucket[o + t] : 0x7fffffff;
#pragma unroll
            for (int i = 0; i < VD_REG; ++i) {
                const int lo = idx < sel[i] ? idx : sel[i];
                const int hi = idx < sel[i] ? sel[i] : idx;
                sel[i] = lo;
                idx = hi;
            }
        }
        float v[VD_REG][NF > 0 ? NF : 1];
        const int any = n > 0 ? sel[0] : 0;              // unused slots re-read a valid row
#pragma unroll
        for (int t = 0; t < VD_REG; ++t) {
            const float* pp = pts + (int64_t)(t < n ? sel[t] : any) * NF;
#pragma unroll
            for (int f = 0; f < NF; ++f) v[t][f] = pp[f];
        }
        float acc[NF > 0 ? NF : 1];
#pragma unroll
        for (int f = 0; f < NF; ++f) acc[f] = 0.f;
#pragma unroll
        for (int t = 0; t < VD_REG; ++t) {
            if (t < n) {
#pragma unroll
                for (int f = 0; f < NF; ++f) acc[f] = vd_step(acc[f], v[t][f], t == 0, reduce);
            }
        }
#pragma unroll
        for (int f = 0; f < NF; ++f) feat[row * NF + f] = reduce == 1 ? acc[f] / denom : acc[f];
        return;
    }
    // any feature count: insertion sort of the lane's own bucket segment (at most VD_REG entries)
    for (int t = 1; t < n; ++t) {
        const int v = bucket[o + t];
        int j = t;
        while (j > 0 && bucket[o + j - 1] > v) { bucket[o + j] = bucket[o + j - 1]; --j; }
        if (j != t) bucket[o + j] = v;
    }
    for (int f = 0; f < nfeat; ++f) {
        float acc = 0.f;
        for (int t = 0; t < n; ++t) acc = vd_step(acc, pts[(int64_t)bucket[o + t] * nfeat + f], t == 0, reduce);
        feat[row * nfeat + f] = reduce == 1 ? acc / denom : acc;
    }
}

// pass 5b: one wave per listed voxel of VD_REG < n <= VD_LIGHT (= 64) points, one index per lane
__global__ __launch_bounds__(256) void vd_wave_kernel(const float* __restrict__ pts, int nfeat, int reduce,
                                                      const int* __restrict__ boff, const int* __restrict__ cnt,
                                                      const int* __restrict__ bucket, const int* __restrict__ mid,
                                                      const int* __restrict__ nmid, float* __restrict__ feat)
{
    const int lane = threadIdx.x & 63;
    const int wave = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6), nwaves = (int)((gridDim.x * blockDim.x) >> 6);
    const int nm = *nmid;
    for (int h = wave; h < nm; h += nwaves) {            // wave-uniform: every lane takes part in the shuffles
        const int row = mid[h];
        const int n = cnt[row], o = boff[row];
        const int idx = lane < n ? bucket[o + lane] : 0x7fffffff;
        // point indices are distinct: an index's rank among the voxel's is its place in ascending order
        int r = 0;
        for (int j = 0; j < n; ++j) r += __builtin_amdgcn_readlane(idx, j) < idx ? 1 : 0;      // j is wave-uniform
        if (lane >= n) r = lane;                         // the unused lanes keep their place: r is a permutation
        const int sorted = __builtin_amdgcn_ds_permute(r << 2, idx);     // lane t holds the t-th smallest index
        for (int f0 = 0; f0 < nfeat; f0 += 8) {          // eight features per round trip to memory
            float val[8];
#pragma unroll
            for (int k = 0; k < 8; ++k)
                val[k] = (lane < n && f0 + k < nfeat) ? pts[(int64_t)sorted * nfeat + f0 + k] : 0.f;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                if (f0 + k < nfeat) {
                    float acc = 0.f;
                    for (int t = 0; t < n; ++t)
                        acc = vd_step(acc, __int_as_float(__builtin_amdgcn_readlane(__float_as_int(val[k]), t)), t == 0,
                                      reduce);
                    if (lane == 0) feat[(int64_t)row * nfeat + f0 + k] = reduce == 1 ? acc / (float)n : acc;
                }
            }
        }
    }
}

// pass 5c: one workgroup per listed voxel of more than VD_LIGHT points
__global__ __launch_bounds__(VD_HEAVY_THREADS) void vd_heavy_kernel(const float* __restrict__ pts, int nfeat, int reduce,
                                                                    const int* __restrict__ boff,
                                                                    const int* __restrict__ cnt,
                                                                    const int* __restrict__ bucket, int* sorted,
                                                                    const int* __restrict__ heavy,
                                                                    const int* __restrict__ nheavy,
                                                                    float* __restrict__ feat)
{
    __shared__ float stage[VD_STAGE_FLOATS];
    const int tid = threadIdx.x;
    const int nh = *nheavy;
    int per = VD_STAGE_FLOATS / nfeat;               // points per stage (nfeat <= VD_MAX_NFEAT: at least 16)
    if (per > VD_HEAVY_THREADS) per = VD_HEAVY_THREADS;
    for (int h = blockIdx.x; h < nh; h += gridDim.x) {
        const int row = heavy[h];
        const int n = cnt[row], o = boff[row];
        // point indices are distinct: an index's rank among the voxel's is its place in ascending order
        for (int e = tid; e < n; e += VD_HEAVY_THREADS) {
            const int mine = bucket[o + e];
            int r = 0;
            for (int j = 0; j < n; ++j) r += bucket[o + j] < mine ? 1 : 0;
            sorted[o + r] = mine;
        }
        __syncthreads();
        float acc = 0.f;
        for (int c0 = 0; c0 < n; c0 += per) {
            const int m = n - c0 < per ? n - c0 : per;
            for (int q = tid; q < m * nfeat; q += VD_HEAVY_THREADS) {
                const int t = q / nfeat, f = q - t * nfeat;
                stage[q] = pts[(int64_t)sorted[o + c0 + t] * nfeat + f];
            }
            __syncthreads();
            if (tid < nfeat)
                for (int t = 0; t < m; ++t) acc = vd_step(acc, stage[t * nfeat + tid], c0 + t == 0, reduce);
            __syncthreads();
        }
        if (tid < nfeat) feat[(int64_t)row * nfeat + tid] = reduce == 1 ? acc / (float)n : acc;
    }
}

// ---------------------------------------------------------------------------------------------------- host side
struct VdWs {
    unsigned* bits; int* gcnt;
    int *pkey, *pframe, *prow, *ppos, *bucket, *sorted, *cnt, *boff, *heavy, *mid, *nlist, *tmp_base;
    void* scan_ws;
    int64_t fgroups, G, bytes;
};

// one presence bit per cell per frame (rounded up to 128-bit groups), a count per group, and arrays per point
static VdWs vd_layout(void* workspace, int64_t npts, int B, int64_t cells)
{
    VdWs w;
    unsigned char* base = (unsigned char*)workspace;
    int64_t o = 0;
    auto take = [&](int64_t bytes) { void* p = base ? (void*)(base + o) : nullptr; o += al3d_align(bytes, 256); return p; };
    w.fgroups = al3d_cdiv(cells, 128);
    w.G = (int64_t)B * w.fgroups;
    w.bits = (unsigned*)take(w.G * 16);
    w.gcnt = (int*)take((w.G + 1) * 4);
    w.pkey = (int*)take(npts * 4);
    w.pframe = (int*)take(npts * 4);
    w.prow = (int*)take(npts * 4);
    w.ppos = (int*)take(npts * 4);
    w.bucket = (int*)take(npts * 4);
    w.sorted = (int*)take(npts * 4);
    w.cnt = (int*)take((npts + 1) * 4);
    w.boff = (int*)take((npts + 1) * 4);
    w.heavy = (int*)take((npts / VD_LIGHT + 1) * 4);     // a listed voxel has more than VD_LIGHT / VD_REG points
    w.mid = (int*)take((npts / VD_REG + 1) * 4);
    w.nlist = (int*)take(8);                             // entries in heavy, in mid
    w.tmp_base = (int*)take(((int64_t)B + 1) * 4);
    w.scan_ws = take(al3d_scan_workspace_bytes((w.G > npts ? w.G : npts) + 1));
    w.bytes = o;
    return w;
}

extern "C" int64_t al3d_voxelize_dynamic_workspace_bytes(int64_t npts, int B, int gx, int gy, int gz)
{
    if (npts < 0 || B < 1 || gx < 1 || gy < 1 || gz < 1) return 0;
    return vd_layout(nullptr, npts, B, (int64_t)gx * gy * gz).bytes;
}

// passes 2-5 behind both front ends: w.bits / w.pkey / w.pframe are filled, *status is initialised
static int vd_rank_and_reduce(const char* who, const float* feats, int64_t npts, int B, int nfeat, VdDims d, int reduce,
                              int64_t rows_cap, const VdWs& w, float* feat, int* coords, int* counts, int* point2voxel,
                              int* num_voxels, int* row_base, int* status, hipStream_t s)
{
    const int64_t nrows = rows_cap < npts ? rows_cap : npts;      // a frame set of npts points has at most npts voxels
    const unsigned pb = (unsigned)al3d_cdiv(npts > 0 ? npts : 1, 256);
    hipLaunchKernelGGL(vd_popc_kernel, dim3((unsigned)al3d_cdiv(w.G + 1, 256)), dim3(256), 0, s, (const uint4*)w.bits, w.G,
                       w.gcnt);
    int rc = al3d_exclusive_scan_i32(w.gcnt, w.gcnt, w.G + 1, w.scan_ws, s);
    if (rc) return rc;
    hipLaunchKernelGGL(vd_base_kernel, dim3(1), dim3(64), 0, s, w.gcnt, w.fgroups, B, rows_cap, num_voxels, row_base,
                       status);
    hipLaunchKernelGGL(vd_assign_kernel, dim3(pb), dim3(256), 0, s, npts, d, w.fgroups * 4, w.bits, w.gcnt, w.pkey,
                       w.pframe, nrows, w.prow, w.ppos, w.cnt, coords, point2voxel);
    rc = al3d_exclusive_scan_i32(w.cnt, w.boff, nrows + 1, w.scan_ws, s);
    if (rc) return rc;
    hipLaunchKernelGGL(vd_bucket_kernel, dim3(pb), dim3(256), 0, s, npts, w.prow, w.ppos, w.boff, w.bucket);
    const unsigned rb = (unsigned)al3d_cdiv(nrows > 0 ? nrows : 1, 128);
#define VD_REDUCE(NF)                                                                                                  \
    hipLaunchKernelGGL((vd_reduce_kernel<NF>), dim3(rb), dim3(128), 0, s, feats, nfeat, reduce, nrows, row_base + B,   \
                       w.boff, w.cnt, w.bucket, feat, counts, w.heavy, w.nlist, w.mid, w.nlist + 1)
    if (nfeat == 5) VD_REDUCE(5);
    else if (nfeat == 4) VD_REDUCE(4);
    else VD_REDUCE(0);
#undef VD_REDUCE
    int64_t mb = al3d_cdiv(npts / VD_REG + 1, 4);                 // four waves per workgroup, one listed voxel per wave
    if (mb > 4096) mb = 4096;
    hipLaunchKernelGGL(vd_wave_kernel, dim3((unsigned)mb), dim3(256), 0, s, feats, nfeat, reduce, w.boff, w.cnt, w.bucket,
                       w.mid, w.nlist + 1, feat);
    int64_t hb = npts / VD_LIGHT + 1;
    if (hb > 1024) hb = 1024;
    hipLaunchKernelGGL(vd_heavy_kernel, dim3((unsigned)hb), dim3(VD_HEAVY_THREADS), 0, s, feats, nfeat, reduce, w.boff,
                       w.cnt, w.bucket, w.sorted, w.heavy, w.nlist, feat);
    AL3D_CHECK_LAUNCH(who);
    return AL3D_OK;
}

static int vd_clear(const char* who, const VdWs& w, int64_t npts, int64_t rows_cap, int* status, hipStream_t s)
{
    const int64_t nrows = rows_cap < npts ? rows_cap : npts;
    if (hipMemsetAsync(w.bits, 0, w.G * 16, s) != hipSuccess || hipMemsetAsync(w.cnt, 0, (nrows + 1) * 4, s) != hipSuccess ||
        hipMemsetAsync(w.nlist, 0, 8, s) != hipSuccess || hipMemsetAsync(status, 0, 4, s) != hipSuccess)
        return al3d_fail(AL3D_ELAUNCH, "%s: memset failed", who);
    return AL3D_OK;
}

extern "C" int al3d_voxelize_dynamic_f32(const float* points, const int64_t* point_offsets, int64_t npts, int B, int nfeat,
                                         const float* range_min, const float* voxel_size, const int* grid_size, int order,
                                         int reduce, int64_t rows_cap, void* workspace, float* feat, int* coords,
                                         int* counts, int* point_coords, int* point2voxel, int* num_voxels, int* row_base,
                                         int* status, void* stream)
{
    const char* who = "al3d_voxelize_dynamic_f32";
    AL3D_REQUIRE(points && point_offsets && range_min && voxel_size && grid_size && workspace && feat && coords &&
                     counts && num_voxels && row_base && status, "%s: null pointer", who);
    AL3D_REQUIRE(order == 0 || order == 1, "%s: order must be 0 (z, y, x) or 1 (x, y, z)", who);
    AL3D_REQUIRE(reduce >= 0 && reduce <= 2, "%s: reduce must be 0 (sum), 1 (mean) or 2 (max)", who);
    AL3D_REQUIRE(B >= 1 && nfeat >= 3 && nfeat <= VD_MAX_NFEAT && npts >= 0 && npts < (1LL << 31) && rows_cap >= 0,
                 "%s: bad sizes (nfeat must be in [3,%d])", who, VD_MAX_NFEAT);
    AL3D_REQUIRE(((uintptr_t)coords & 15) == 0 && ((uintptr_t)points & 3) == 0,
                 "%s: coords must be 16-byte aligned (one int4 per voxel), points 4-byte aligned", who);
    VoxCfg c;
    c.min_x = range_min[0]; c.min_y = range_min[1]; c.min_z = range_min[2];
    c.vs_x = voxel_size[0]; c.vs_y = voxel_size[1]; c.vs_z = voxel_size[2];
    c.gx = grid_size[0]; c.gy = grid_size[1]; c.gz = grid_size[2];
    c.max_points = 0; c.max_voxels = 0; c.nfeat = nfeat;
    AL3D_REQUIRE(c.gx >= 1 && c.gy >= 1 && c.gz >= 1, "%s: bad grid", who);
    const int64_t cells = (int64_t)c.gx * c.gy * c.gz;
    AL3D_REQUIRE(cells < (1LL << 31), "%s: grid too large (gx*gy*gz must be below 2^31)", who);
    const VdWs w = vd_layout(workspace, npts, B, cells);
    AL3D_REQUIRE(w.G + 1 < (1LL << 31), "%s: batch x grid too large", who);
    hipStream_t s = (hipStream_t)stream;
    int rc = vd_clear(who, w, npts, rows_cap, status, s);
    if (rc) return rc;
    hipLaunchKernelGGL(vd_key_points_kernel, dim3((unsigned)al3d_cdiv(npts > 0 ? npts : 1, 256)), dim3(256), 0, s, points,
                       point_offsets, B, npts, c, order, w.fgroups * 4, w.bits, w.pkey, w.pframe, point_coords);
    VdDims d;
    if (order == 0) { d.d0 = c.gz; d.d1 = c.gy; d.d2 = c.gx; } else { d.d0 = c.gx; d.d1 = c.gy; d.d2 = c.gz; }
    d.ncol = 4;
    return vd_rank_and_reduce(who, points, npts, B, nfeat, d, reduce, rows_cap, w, feat, coords, counts, point2voxel,
                              num_voxels, row_base, status, s);
}

extern "C" int al3d_dynamic_scatter_f32(const float* feats, const int* coors, int64_t n, int nfeat, const int* dims,
                                        int reduce, int64_t rows_cap, void* workspace, float* out_feats, int* out_coors,
                                        int* counts, int* point2voxel, int* num_voxels, int* status, void* stream)
{
    const char* who = "al3d_dynamic_scatter_f32";
    AL3D_REQUIRE(feats && coors && dims && workspace && out_feats && out_coors && counts && num_voxels && status,
                 "%s: null pointer", who);
    AL3D_REQUIRE(reduce >= 0 && reduce <= 2, "%s: reduce must be 0 (sum), 1 (mean) or 2 (max)", who);
    AL3D_REQUIRE(nfeat >= 1 && nfeat <= VD_MAX_NFEAT && n >= 0 && n < (1LL << 31) && rows_cap >= 0,
                 "%s: bad sizes (nfeat must be in [1,%d])", who, VD_MAX_NFEAT);
    VdDims d;
    d.d0 = dims[0]; d.d1 = dims[1]; d.d2 = dims[2]; d.ncol = 3;
    AL3D_REQUIRE(d.d0 >= 1 && d.d1 >= 1 && d.d2 >= 1, "%s: bad extents", who);
    const int64_t cells = (int64_t)d.d0 * d.d1 * d.d2;
    AL3D_REQUIRE(cells < (1LL << 31), "%s: extents too large (their product must be below 2^31)", who);
    const VdWs w = vd_layout(workspace, n, 1, cells);
    hipStream_t s = (hipStream_t)stream;
    int rc = vd_clear(who, w, n, rows_cap, status, s);
    if (rc) return rc;
    hipLaunchKernelGGL(vd_key_coors_kernel, dim3((unsigned)al3d_cdiv(n > 0 ? n : 1, 256)), dim3(256), 0, s, coors, n, d,
                       w.bits, w.pkey, w.pframe, status);
    // rows before frame 0 and the total land in workspace words; the caller reads the total from num_voxels[0]
    return vd_rank_and_reduce(who, feats, n, 1, nfeat, d, reduce, rows_cap, w, out_feats, out_coors, counts, point2voxel,
                              num_voxels, w.tmp_base, status, s);
}
