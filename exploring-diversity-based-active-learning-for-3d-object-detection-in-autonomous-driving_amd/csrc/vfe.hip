// Fused VFE reader: det3d's learned voxel feature extractor in one launch (fp32 on the VALU, deterministic, no atomics).
//
// Replaces VoxelFeatureExtractor.forward / VoxelFeatureExtractorV2.forward + VFELayer.forward
// (det3d/models/readers/voxel_encoder.py:13-176) in eval mode with BatchNorm folded to scale / shift.
//
// Per voxel, n = num_points clipped to [0, T]:
//   - mean = (f32 sum of xyz over slots 0..n-1 in ascending slot order) / (float)max(n, 1).
//   - slot p < n is decorated [f_0..f_{F-1}, xyz - mean, (|xyz|)].
//   - slots p >= n are NOT masked in front of the first layer (the reference multiplies by the mask only after vfe1,
//     voxel_encoder.py:98-99), so each enters vfe1 as [0..0, -mean, (0)].  All T - n of them are identical: one
//     representative row stands for them in vfe1's max.  After vfe1 the padded rows are zero (pointwise and repeated max
//     alike), so in vfe2 they hold relu(b2) and join its max; after the last linear they are zero again and the final
//     max runs over the real rows and, when n < T, one 0.  n = 0 (the reference gives NaN there): every slot is padded,
//     the row is 0.
//   - layer l: h = relu(fma(dot, s_l, b_l)), dot accumulated by fmaf in ascending k; agg = max over the T slots; the next
//     layer reads [h, agg].
//   - NaN input (a deviation: the reference's relu / max give the voxel a NaN row).  ReLU is fmaxf(pre, 0), which drops a
//     NaN operand, so a NaN pre-activation gives 0 and no NaN outlives vfe1.  A NaN in a feature past xyz makes its own
//     slot's vfe1 pre-activations NaN in every unit (NaN * w is NaN, whatever w): that slot's vfe1 row is 0, the others
//     are untouched.  A NaN in x, y or z also makes the mean NaN and with it xyz - mean of every real slot and -mean of
//     the padded representative: all vfe1 rows and vfe1's max are 0, and the voxel goes on as if vfe1 had given 0
//     everywhere.  The row is finite either way; other voxels are never touched.  inf follows IEEE arithmetic through
//     the chains (inf - inf and 0 * inf give NaN, then the rule above) and is not pinned beyond staying in its voxel.
//
// Shape: persistent workgroups of up to eight wave64, all folded weights resident in LDS (w3 alone is 64 KB at C = 128).
// A wave takes V consecutive voxels at a time and keeps their rows in its own LDS region; nothing per slot goes to HBM.
// In every layer a lane owns FOUR consecutive units (one 16-byte weight read per k) of one voxel and RC = 8 (or 4) of its
// rows in registers: per four k that is 4 weight reads + RC activation reads (16 bytes each, a broadcast inside the lane
// group) for 16 * RC FMAs, and the repeated max half of the input is read once for all RC rows.  U / 4 lanes cover a
// layer's units, so 64 / (U / 4) voxels run side by side; a voxel's max stays in its lanes' registers.
// A row's value is one fixed fmaf chain whatever V, RC, the block count or the voxel's place in the batch: the same bits.
#include "al3d_common.h"

struct VfeArgs {
    const float* voxels;     // [M, T, F]
    const int* num_points;   // [M]
    const float *w1, *s1, *b1;   // [K1, U1]
    const float *w2, *s2, *b2;   // [2*U1, U2] or null
    const float *w3, *s3, *b3;   // [C, C]
    float* out;              // [M, C]
    int64_t M;
    int T, F, wd, K1, K1p, U1, U2, C, V;
    int per_wave;            // floats of one wave's LDS region
};

__device__ __forceinline__ void vfe_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// acc[j][c] = sum over k of x_j[k] * w[k][4*ul + c], k ascending: KA values of row j (xa + min(j, nvalid-1) * lda), then
// KB values shared by all rows (xb).  KA, KB multiples of 4; rows at or past nvalid repeat the last valid row (discarded).
template <int RC>
__device__ __forceinline__ void vfe_chunk(const float* xa, int lda, int KA, const float* xb, int KB, const float* w,
                                          int U4, int ul, int nvalid, float (&acc)[RC][4])
{
    const float* xr[RC];
#pragma unroll
    for (int j = 0; j < RC; ++j) {
        xr[j] = xa + (j < nvalid ? j : nvalid - 1) * lda;
        acc[j][0] = acc[j][1] = acc[j][2] = acc[j][3] = 0.f;
    }
    const float4* W = reinterpret_cast<const float4*>(w) + ul;
    for (int k = 0; k < KA; k += 4) {
        const float4 w0 = W[(k + 0) * U4], w1 = W[(k + 1) * U4], w2 = W[(k + 2) * U4], w3 = W[(k + 3) * U4];
#pragma unroll
        for (int j = 0; j < RC; ++j) {
            const float4 a = *reinterpret_cast<const float4*>(xr[j] + k);
            acc[j][0] = fmaf(a.x, w0.x, acc[j][0]); acc[j][1] = fmaf(a.x, w0.y, acc[j][1]);
            acc[j][2] = fmaf(a.x, w0.z, acc[j][2]); acc[j][3] = fmaf(a.x, w0.w, acc[j][3]);
            acc[j][0] = fmaf(a.y, w1.x, acc[j][0]); acc[j][1] = fmaf(a.y, w1.y, acc[j][1]);
            acc[j][2] = fmaf(a.y, w1.z, acc[j][2]); acc[j][3] = fmaf(a.y, w1.w, acc[j][3]);
            acc[j][0] = fmaf(a.z, w2.x, acc[j][0]); acc[j][1] = fmaf(a.z, w2.y, acc[j][1]);
            acc[j][2] = fmaf(a.z, w2.z, acc[j][2]); acc[j][3] = fmaf(a.z, w2.w, acc[j][3]);
            acc[j][0] = fmaf(a.w, w3.x, acc[j][0]); acc[j][1] = fmaf(a.w, w3.y, acc[j][1]);
            acc[j][2] = fmaf(a.w, w3.z, acc[j][2]); acc[j][3] = fmaf(a.w, w3.w, acc[j][3]);
        }
    }
    W += (size_t)KA * U4;
    for (int k = 0; k < KB; k += 4) {
        const float4 w0 = W[(k + 0) * U4], w1 = W[(k + 1) * U4], w2 = W[(k + 2) * U4], w3 = W[(k + 3) * U4];
        const float4 a = *reinterpret_cast<const float4*>(xb + k);
#pragma unroll
        for (int j = 0; j < RC; ++j) {
            acc[j][0] = fmaf(a.x, w0.x, acc[j][0]); acc[j][1] = fmaf(a.x, w0.y, acc[j][1]);
            acc[j][2] = fmaf(a.x, w0.z, acc[j][2]); acc[j][3] = fmaf(a.x, w0.w, acc[j][3]);
            acc[j][0] = fmaf(a.y, w1.x, acc[j][0]); acc[j][1] = fmaf(a.y, w1.y, acc[j][1]);
            acc[j][2] = fmaf(a.y, w1.z, acc[j][2]); acc[j][3] = fmaf(a.y, w1.w, acc[j][3]);
            acc[j][0] = fmaf(a.z, w2.x, acc[j][0]); acc[j][1] = fmaf(a.z, w2.y, acc[j][1]);
            acc[j][2] = fmaf(a.z, w2.z, acc[j][2]); acc[j][3] = fmaf(a.z, w2.w, acc[j][3]);
            acc[j][0] = fmaf(a.w, w3.x, acc[j][0]); acc[j][1] = fmaf(a.w, w3.y, acc[j][1]);
            acc[j][2] = fmaf(a.w, w3.z, acc[j][2]); acc[j][3] = fmaf(a.w, w3.w, acc[j][3]);
        }
    }
}

// relu(fma(acc, s, b)) of the chunk's rows r0 + j < nr: rows below nstore go to hrow (LDS, ldh apart), all join mx
template <int RC>
__device__ __forceinline__ void vfe_epilogue(const float (&acc)[RC][4], const float4 sc, const float4 sh, int r0, int nr,
                                             int nstore, float* hrow, int ldh, float4& mx)
{
#pragma unroll
    for (int j = 0; j < RC; ++j) {
        const int r = r0 + j;
        if (r < nr) {
            float4 v;
            v.x = fmaxf(fmaf(acc[j][0], sc.x, sh.x), 0.f);
            v.y = fmaxf(fmaf(acc[j][1], sc.y, sh.y), 0.f);
            v.z = fmaxf(fmaf(acc[j][2], sc.z, sh.z), 0.f);
            v.w = fmaxf(fmaf(acc[j][3], sc.w, sh.w), 0.f);
            if (r < nstore) *reinterpret_cast<float4*>(hrow + r * ldh) = v;
            mx.x = fmaxf(mx.x, v.x); mx.y = fmaxf(mx.y, v.y); mx.z = fmaxf(mx.z, v.z); mx.w = fmaxf(mx.w, v.w);
        }
    }
}

// One layer over the wave's V voxels.  Voxel v reads rows xa + v * xa_vox (lda apart, KA wide) and the shared half
// xb + v * xb_vox (KB wide); nr(v) = n + extra_row * (n < T) rows are computed, the first n stored to hout; pad_join: a
// padded slot's value relu(fma(0, s, b)) joins the max when n < T.  The max goes to agg (LDS, U apart) or to gout
// (global, rows of the live voxels).
__device__ __forceinline__ void vfe_layer(const float* xa, int xa_vox, int lda, int KA, const float* xb, int xb_vox, int KB,
                                          const float* w, const float* s, const float* b, int U, const int* nn, int V,
                                          int T, bool extra_row, bool pad_join, float* hout, int h_vox, int ldh,
                                          float* agg, float* gout, int64_t base, int64_t M, int lane)
{
    const int U4 = U >> 2, NG = 64 / U4, g = lane / U4, ul = lane - g * U4;
    if (g >= NG) return;
    const float4 sc = reinterpret_cast<const float4*>(s)[ul], sh = reinterpret_cast<const float4*>(b)[ul];
    for (int v = g; v < V; v += NG) {
        const int n = nn[v];
        const int nr = n + ((extra_row && n < T) ? 1 : 0);
        float4 mx = make_float4(0.f, 0.f, 0.f, 0.f);      // every value is a relu output, >= 0
        if (pad_join && n < T) {
            mx.x = fmaxf(fmaf(0.f, sc.x, sh.x), 0.f); mx.y = fmaxf(fmaf(0.f, sc.y, sh.y), 0.f);
            mx.z = fmaxf(fmaf(0.f, sc.z, sh.z), 0.f); mx.w = fmaxf(fmaf(0.f, sc.w, sh.w), 0.f);
        }
        const float* xv = xa + v * xa_vox;
        const float* bv = xb + v * xb_vox;
        float* hv = hout ? hout + v * h_vox + 4 * ul : nullptr;
        const int nstore = hout ? n : 0;
        int r0 = 0;
        for (; nr - r0 > 4; r0 += 8) {
            float acc[8][4];
            vfe_chunk<8>(xv + r0 * lda, lda, KA, bv, KB, w, U4, ul, nr - r0, acc);
            vfe_epilogue<8>(acc, sc, sh, r0, nr, nstore, hv, ldh, mx);
        }
        if (r0 < nr) {
            float acc[4][4];
            vfe_chunk<4>(xv + r0 * lda, lda, KA, bv, KB, w, U4, ul, nr - r0, acc);
            vfe_epilogue<4>(acc, sc, sh, r0, nr, nstore, hv, ldh, mx);
        }
        if (agg) *reinterpret_cast<float4*>(agg + v * U + 4 * ul) = mx;
        if (gout && base + v < M) *reinterpret_cast<float4*>(gout + (base + v) * U + 4 * ul) = mx;
    }
}

__global__ __launch_bounds__(512) void vfe_net_kernel(VfeArgs a)
{
    extern __shared__ float4 vfe_lds4[];
    float* lds = reinterpret_cast<float*>(vfe_lds4);
    const int wpb = blockDim.x >> 6, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int T = a.T, F = a.F, K1 = a.K1, K1p = a.K1p, U1 = a.U1, U2 = a.U2, C = a.C, V = a.V;
    const bool two = U2 > 0;
    // resident weights (every offset a multiple of 4 floats)
    float* w1 = lds;
    float* s1 = w1 + K1p * U1;
    float* b1 = s1 + U1;
    float* w2 = b1 + U1;
    float* s2 = w2 + (two ? 2 * U1 * U2 : 0);
    float* b2 = s2 + U2;
    float* w3 = b2 + U2;
    float* s3 = w3 + C * C;
    float* b3 = s3 + C;
    // this wave's rows
    const int ld1 = U1 + 4, ld2 = U2 + 4;
    float* x1 = b3 + C + wave * a.per_wave;          // [V][T][K1p] decorated slots (row n: the padded-slot representative)
    float* mean = x1 + V * T * K1p;                  // [V][4]
    float* h1 = mean + V * 4;                        // [V][T][U1+4]
    float* a1 = h1 + V * T * ld1;                    // [V][U1]
    float* h2 = a1 + V * U1;                         // [V][T][U2+4]
    float* a2 = h2 + V * T * ld2;                    // [V][U2]
    int* nn = reinterpret_cast<int*>(a2 + V * U2);   // [V]

    for (int i = threadIdx.x; i < K1p * U1; i += blockDim.x) w1[i] = i < K1 * U1 ? a.w1[i] : 0.f;
    for (int i = threadIdx.x; i < U1; i += blockDim.x) { s1[i] = a.s1[i]; b1[i] = a.b1[i]; }
    if (two) {
        for (int i = threadIdx.x; i < 2 * U1 * U2; i += blockDim.x) w2[i] = a.w2[i];
        for (int i = threadIdx.x; i < U2; i += blockDim.x) { s2[i] = a.s2[i]; b2[i] = a.b2[i]; }
    }
    for (int i = threadIdx.x; i < C * C; i += blockDim.x) w3[i] = a.w3[i];
    for (int i = threadIdx.x; i < C; i += blockDim.x) { s3[i] = a.s3[i]; b3[i] = a.b3[i]; }
    __syncthreads();

    // from here on a wave touches its own LDS region only: wave-level synchronisation
    const int64_t ngroups = (a.M + V - 1) / V;
    for (int64_t grp = (int64_t)blockIdx.x * wpb + wave; grp < ngroups; grp += (int64_t)gridDim.x * wpb) {
        const int64_t base = grp * V;
        if (lane < V) {
            int n = base + lane < a.M ? a.num_points[base + lane] : 0;
            nn[lane] = n < 0 ? 0 : (n > T ? T : n);
        }
        vfe_wave_sync();
        // raw slots (real ones only), zero-padded to K1p
        for (int i = lane; i < V * T; i += 64) {
            const int v = i / T, p = i - v * T;
            float* row = x1 + i * K1p;
            if (p < nn[v]) {
                const float* src = a.voxels + ((base + v) * T + p) * F;
                for (int f = 0; f < F; ++f) row[f] = src[f];
                for (int f = F; f < K1p; ++f) row[f] = 0.f;
            }
        }
        vfe_wave_sync();
        if (lane < V) {
            const int n = nn[lane];
            const float* rows = x1 + lane * T * K1p;
            float mx = 0.f, my = 0.f, mz = 0.f;
            for (int p = 0; p < n; ++p) { mx += rows[p * K1p]; my += rows[p * K1p + 1]; mz += rows[p * K1p + 2]; }
            const float d = (float)(n > 0 ? n : 1);
            mean[lane * 4 + 0] = mx / d; mean[lane * 4 + 1] = my / d; mean[lane * 4 + 2] = mz / d;
        }
        vfe_wave_sync();
        for (int i = lane; i < V * T; i += 64) {
            const int v = i / T, p = i - v * T, n = nn[v];
            float* row = x1 + i * K1p;
            const float mx = mean[v * 4], my = mean[v * 4 + 1], mz = mean[v * 4 + 2];
            if (p < n) {
                const float x = row[0], y = row[1], z = row[2];
                row[F + 0] = x - mx; row[F + 1] = y - my; row[F + 2] = z - mz;
                if (a.wd) row[F + 3] = sqrtf(x * x + y * y + z * z);
            } else if (p == n) {                         // n < T: the representative of the T - n padded slots
                for (int f = 0; f < K1p; ++f) row[f] = 0.f;
                row[F + 0] = 0.f - mx; row[F + 1] = 0.f - my; row[F + 2] = 0.f - mz;
            }
        }
        vfe_wave_sync();
        // vfe1: rows 0..n-1 and the padded representative; the padded rows are zeroed afterwards (not stored)
        vfe_layer(x1, T * K1p, K1p, K1p, x1, 0, 0, w1, s1, b1, U1, nn, V, T, true, false, h1, T * ld1, ld1, a1, nullptr,
                  base, a.M, lane);
        vfe_wave_sync();
        if (two) {
            // vfe2: the real rows read [h1, agg1]; a padded slot reads zeros and holds relu(b2)
            vfe_layer(h1, T * ld1, ld1, U1, a1, U1, U1, w2, s2, b2, U2, nn, V, T, false, true, h2, T * ld2, ld2, a2, nullptr,
                      base, a.M, lane);
            vfe_wave_sync();
            vfe_layer(h2, T * ld2, ld2, U2, a2, U2, U2, w3, s3, b3, C, nn, V, T, false, false, nullptr, 0, 0, nullptr, a.out,
                      base, a.M, lane);
        } else {
            vfe_layer(h1, T * ld1, ld1, U1, a1, U1, U1, w3, s3, b3, C, nn, V, T, false, false, nullptr, 0, 0, nullptr, a.out,
                      base, a.M, lane);
        }
        vfe_wave_sync();
    }
}

static int vfe_launch(VfeArgs a, int voxels_per_wave, int max_blocks, void* stream, const char* name)
{
    AL3D_REQUIRE(a.M >= 0, "%s: M %lld must be >= 0", name, (long long)a.M);
    AL3D_REQUIRE(a.T >= 1 && a.T <= 64, "%s: T %d: need 1 <= T <= 64", name, a.T);
    AL3D_REQUIRE(a.F >= 3 && a.F <= 10, "%s: F %d: need 3 <= F <= 10", name, a.F);
    AL3D_REQUIRE(a.U1 >= 16 && a.U1 <= 64 && a.U1 % 16 == 0, "%s: layer 1 units %d: need a multiple of 16 in [16, 64]",
                 name, a.U1);
    if (a.w2) {
        AL3D_REQUIRE(a.U2 >= 16 && a.U2 <= 64 && a.U2 % 16 == 0,
                     "%s: layer 2 units %d: need a multiple of 16 in [16, 64]", name, a.U2);
        AL3D_REQUIRE(a.s2 && a.b2, "%s: layer 2 scale/shift missing", name);
    } else {
        a.U2 = 0;
    }
    const int last = a.w2 ? a.U2 : a.U1;
    AL3D_REQUIRE(a.C == 2 * last, "%s: C %d must be twice the last VFE layer's units (%d)", name, a.C, last);
    AL3D_REQUIRE(a.w1 && a.s1 && a.b1 && a.w3 && a.s3 && a.b3, "%s: null weight pointer", name);
    AL3D_REQUIRE(voxels_per_wave >= 0 && voxels_per_wave <= 16 && max_blocks >= 0,
                 "%s: launch shape (voxels_per_wave %d, max_blocks %d): need 0 <= voxels_per_wave <= 16, max_blocks >= 0",
                 name, voxels_per_wave, max_blocks);
    AL3D_REQUIRE(a.M == 0 || (a.voxels && a.num_points && a.out), "%s: null pointer", name);
    if (a.M == 0) return AL3D_OK;
    a.wd = a.wd ? 1 : 0;
    a.K1 = a.F + 3 + a.wd;
    a.K1p = (a.K1 + 3) & ~3;
    const int64_t fixed = (int64_t)a.K1p * a.U1 + 2 * a.U1 + (a.w2 ? 2 * a.U1 * a.U2 : 0) + 2 * a.U2 +
                          (int64_t)a.C * a.C + 2 * a.C;
    const int64_t per_voxel = (int64_t)a.T * a.K1p + 4 + (int64_t)a.T * (a.U1 + 4) + a.U1 +
                              (int64_t)a.T * (a.U2 + 4) + a.U2;
    const int64_t limit = 160 * 1024;
    int V = voxels_per_wave ? voxels_per_wave : 2, wpb = 8;
    auto region = [&](int v) { return al3d_align(v * per_voxel + v, 4); };      // + the clipped counts
    while ((fixed + wpb * region(V)) * 4 > limit && (V > 1 || wpb > 1)) {
        if (V > 1) --V; else wpb >>= 1;
    }
    const int64_t bytes = (fixed + wpb * region(V)) * 4;
    AL3D_REQUIRE(bytes <= limit, "%s: %lld bytes of LDS needed (> 160 KiB)", name, (long long)bytes);
    a.V = V;
    a.per_wave = (int)region(V);
    if (bytes > 64 * 1024 &&
        hipFuncSetAttribute((const void*)vfe_net_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)limit) !=
            hipSuccess)
        return al3d_fail(AL3D_ELAUNCH, "%s: cannot raise the LDS limit", name);
    if (max_blocks == 0) {
        int dev = 0, cus = 0;
        if (hipGetDevice(&dev) != hipSuccess ||
            hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1)
            return al3d_fail(AL3D_ELAUNCH, "%s: cannot read the compute-unit count", name);
        int per_cu = (int)(limit / bytes);
        max_blocks = cus * (per_cu < 1 ? 1 : (per_cu > 4 ? 4 : per_cu));      // persistent: what fits on the chip at once
    }
    const int64_t blocks = al3d_cdiv(al3d_cdiv(a.M, V), wpb);
    const int grid = (int)(blocks < max_blocks ? blocks : max_blocks);
    hipLaunchKernelGGL(vfe_net_kernel, dim3(grid), dim3(64 * wpb), (size_t)bytes, (hipStream_t)stream, a);
    AL3D_CHECK_LAUNCH("vfe_net_kernel");
    return AL3D_OK;
}

extern "C" int al3d_vfe_net_launch_f32(const float* voxels, const int* num_points, int64_t M, int T, int F,
                                       int with_distance, const float* w1, const float* s1, const float* b1, int U1,
                                       const float* w2, const float* s2, const float* b2, int U2, const float* w3,
                                       const float* s3, const float* b3, int C, float* out, int voxels_per_wave,
                                       int max_blocks, void* stream)
{
    VfeArgs a{voxels, num_points, w1, s1, b1, w2, s2, b2, w3, s3, b3, out, M, T, F, with_distance, 0, 0, U1, U2, C, 0, 0};
    return vfe_launch(a, voxels_per_wave, max_blocks, stream, "al3d_vfe_net_launch_f32");
}

extern "C" int al3d_vfe_net_f32(const float* voxels, const int* num_points, int64_t M, int T, int F, int with_distance,
                                const float* w1, const float* s1, const float* b1, int U1, const float* w2,
                                const float* s2, const float* b2, int U2, const float* w3, const float* s3,
                                const float* b3, int C, float* out, void* stream)
{
    VfeArgs a{voxels, num_points, w1, s1, b1, w2, s2, b2, w3, s3, b3, out, M, T, F, with_distance, 0, 0, U1, U2, C, 0, 0};
    return vfe_launch(a, 0, 0, stream, "al3d_vfe_net_f32");
}
