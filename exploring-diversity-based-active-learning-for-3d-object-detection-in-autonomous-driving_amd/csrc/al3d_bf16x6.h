// The bf16x6 arithmetic: fp32-faithful products on the bf16 matrix cores (gfx950).  Device-only; the one definition
// behind conv2d_bf16x6.hip, spconv_bf16x6.hip, spconv_wave.hip and tokens_bf16x6.hip.
//
// Every fp32 operand is split exactly into three bf16 pieces x = x1 + x2 + x3 (8+8+8 significand bits); a product x*w
// is formed as the six partial products of total order <= 2 (x3w1, x2w2, x1w3, x2w1, x1w2, x1w1), each exact in fp32,
// accumulated smallest first into ONE fp32 accumulator by v_mfma_f32_32x32x16_bf16.  The three dropped terms are below
// 2^-25 |x w| -- smaller than the rounding of the fp32 product itself -- so results agree with an fp32 FMA chain to
// fp32 rounding noise (the tests compare against fp64 references).  bf16 has fp32's exponent: no operand needs a range
// check and no piece a power-of-two lift.  Six bf16 MFMAs cost 6/16 of the fp32-input MFMA they replace (MI355X:
// v_mfma_f32_32x32x2_f32 runs at 1/16 of the bf16 rate), i.e. up to 2.67x the fp32 matrix-core roof.
//
// Whoever changes the split or the product order changes it here, for every kernel at once.
#pragma once
#include "conv2d_tile.h"      // f32x16, mfma32_crow

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));

// Bytes per staged LDS row of 16 channels: 16 bf16 (32 B) + 16 B pad.  At a 48-byte pitch the 32 rows x 2 halves that
// the lanes of a fragment read with one ds_read_b128 fall on distinct bank groups (conflict-free); at 32 they collide.
#define B6_PITCH 48

// x = a + b + c exactly.  Not pinned: where the producer's arithmetic is visible to the compiler (the token attention),
// the caller pins x first (tokens_bf16x6.hip, tb_split); the staged loaders split loaded values and a pin only costs
// them their packed subtractions.  spconv_wave.hip has a pair-wise form of the same split (sw_split8, same bits) for
// operands split in registers right next to MFMAs under -fno-slp-vectorize.
__device__ __forceinline__ void b6_split(float x, __bf16& a, __bf16& b, __bf16& c)
{
    a = (__bf16)x;
    const float r1 = x - (float)a;
    b = (__bf16)r1;
    const float r2 = r1 - (float)b;
    c = (__bf16)r2;
}

// an MFMA operand fragment of 8 fp32 values: its three planes
struct B6Frag {
    bf16x8 p[3];            // hi, mid, lo
};

// The t-th of the six products, t = 0..5 in accumulation order (smallest first).  t must be a compile-time constant
// after unrolling.  A kernel that interleaves several tiles product-major (the halo kernel) loops over t itself.
__device__ __forceinline__ void b6_product(int t, const B6Frag& a, const B6Frag& b, f32x16& acc)
{
    constexpr int PA[6] = {2, 1, 0, 1, 0, 0}, PB[6] = {0, 1, 2, 0, 1, 0};
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.p[PA[t]], b.p[PB[t]], acc, 0, 0, 0);
}
// acc += A B over one 16-channel step
__device__ __forceinline__ void b6_mac6(const B6Frag& a, const B6Frag& b, f32x16& acc)
{
#pragma unroll
    for (int t = 0; t < 6; ++t) b6_product(t, a, b, acc);
}

// ---- staging through LDS: planes[3][rows * pitch], a row = 16 channels
// split four staged floats (channels 4q .. 4q+3 of a row; off = row * B6_PITCH + 8 * q) into the three planes.
// SPLIT is b6_split for every caller but the token GEMM, which keeps its pinned wrapper (and with it its code).
typedef void (*B6SplitFn)(float, __bf16&, __bf16&, __bf16&);
template <B6SplitFn SPLIT = b6_split, int N>
__device__ __forceinline__ void b6_stage4(unsigned char (&planes)[3][N], int off, const float4& f)
{
    const float v[4] = {f.x, f.y, f.z, f.w};
    bf16x4 h, m, l;
#pragma unroll
    for (int e = 0; e < 4; ++e) { __bf16 a, b, c; SPLIT(v[e], a, b, c); h[e] = a; m[e] = b; l[e] = c; }
    *reinterpret_cast<bf16x4*>(&planes[0][off]) = h;
    *reinterpret_cast<bf16x4*>(&planes[1][off]) = m;
    *reinterpret_cast<bf16x4*>(&planes[2][off]) = l;
}
// the fragment at (row, half) of B6_PITCH rows: lane (fr, fh) of a 32-row tile reads row = tile row + fr, half = fh
template <int N>
__device__ __forceinline__ B6Frag b6_frag(const unsigned char (&planes)[3][N], int row, int half)
{
    B6Frag f;
#pragma unroll
    for (int pl = 0; pl < 3; ++pl) f.p[pl] = *reinterpret_cast<const bf16x8*>(&planes[pl][row * B6_PITCH + 16 * half]);
    return f;
}

// C fragment of v_mfma_f32_32x32x16: lane (fr, fh) holds column fr; register r holds this row of the tile
__device__ __forceinline__ int b6_crow(int r, int fh) { return mfma32_crow(r, fh); }      // conv2d_tile.h

// ---- the staged 128 x 128 x 16 tile pipeline (256 threads: four waves of 64 x 64, wave w = (wm, wn) = (w & 1, w >> 1))
// acc[i][j] += A B over nsteps 16-channel steps, A and B rows staged through double-buffered LDS
// [buf][A|B][plane][row * 48 B]: load step s+1 into registers, read the fragments of step s, 24 MFMAs, store s+1, barrier.
//   load_a(s, row, q, ra): ra[i] = channels 4q .. 4q+3 of A row `row + 64 i` (row 0..63) at step s, or zeros
//   load_b(s, row, q, rb): rb[pl] = bf16 channels 8q .. 8q+7 of plane pl of B row `row` (0..127) at step s, or zeros
// (a thread's whole share of an operand in one call: what is common to it -- the position of step s, the bounds test of
// the B row -- is then worked out once, outside the exec-masked loads)
// (Loading the pre-split weight fragments straight from L2 into registers instead of staging them was measured 17 %
// slower: fragment-shaped loads touch 32 lines for 1 KiB.)
template <B6SplitFn SPLIT = b6_split, class LoadA, class LoadB>
__device__ __forceinline__ void b6_tile_pipeline(int nsteps, LoadA load_a, LoadB load_b, f32x16 (&acc)[2][2])
{
    __shared__ __attribute__((aligned(16))) unsigned char lds[2][2][3][128 * B6_PITCH];
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int wm = wave & 1, wn = wave >> 1;
    const int fr = lane & 31, fh = lane >> 5;
    // A staging: 128 rows x 16 ch f32 = 4 float4 per row -> 512 float4, 2 per thread
    const int aq = tid & 3, ar = tid >> 2;            // piece, row (0..63), +64 on pass 1
    // B staging: per plane 128 rows x 16 bf16 = 2 x 16 B per row -> 256 pieces, 1 per thread
    const int bq = tid & 1, br = tid >> 1;

    float4 ra[2];
    uint4 rb[3];
    auto load_step = [&](int step) {
        load_a(step, ar, aq, ra);
        load_b(step, br, bq, rb);
    };
    auto store_step = [&](int buf) {
#pragma unroll
        for (int i = 0; i < 2; ++i) b6_stage4<SPLIT>(lds[buf][0], (ar + 64 * i) * B6_PITCH + 8 * aq, ra[i]);
#pragma unroll
        for (int pl = 0; pl < 3; ++pl)
            *reinterpret_cast<uint4*>(&lds[buf][1][pl][br * B6_PITCH + 16 * bq]) = rb[pl];
    };

#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    load_step(0);
    store_step(0);
    __syncthreads();
    for (int step = 0; step < nsteps; ++step) {
        const int buf = step & 1;
        if (step + 1 < nsteps) load_step(step + 1);
        B6Frag a[2], b[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            a[t] = b6_frag(lds[buf][0], wm * 64 + t * 32 + fr, fh);
            b[t] = b6_frag(lds[buf][1], wn * 64 + t * 32 + fr, fh);
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) b6_mac6(a[i], b[j], acc[i][j]);
        if (step + 1 < nsteps) store_step(buf ^ 1);
        __syncthreads();
    }
}
