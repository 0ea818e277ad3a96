// Token-matrix kernels in fp32-faithful bf16x6 arithmetic (AL3D_MATH=bf16x6 / f32 on the token path): the token GEMM,
// the 7 x 7 window attention (both row orders) and the head-dim-16 attention of tokens.hip with every matrix product
// formed as in conv2d_bf16x6.hip -- each fp32 operand split exactly into three bf16 pieces x = x1 + x2 + x3, a product
// as the six partial products of total order <= 2 (x1w1, x1w2, x2w1, x1w3, x2w2, x3w1), accumulated in fp32 by
// v_mfma_f32_32x32x16_bf16, smallest first.  bf16 has fp32's exponent: no operand needs |x| < 65504, no piece needs a
// power-of-two lift, and all six products go into ONE accumulator.  The bf16 product has the fragment shapes of the f16
// one, so row / lane orders, the staged-row swizzle, the softmax down the accumulator registers and the chunk combine
// are those of tokens.hip (tok_shared.h).  f32 rows in and out: pair rows are f16 planes and do not exist here.
//
//   tok_linear_bf16x6_kernel            128 x 128 x 16 tile staged through LDS like conv2d_bf16x6_kernel; activations
//                                       split while they are staged, weights pre-split [3][N][K]; epilogue: scale,
//                                       bias, exact GELU / ReLU, residual, row scatter
//   tok_window_attention_bf16x6_kernel  q (scaled), k, v and the probabilities split three ways; softmax in fp32 VALU
//   tok_mha16_bf16x6_kernel             the same for 16-channel heads, chunked online softmax, + the shared combine
//
// Written for correctness over the full fp32 range, not for speed.  gfx950 only.
#include "al3d_common.h"
#include "tok_shared.h"

typedef __bf16 tb_bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 tb_bf16x4 __attribute__((ext_vector_type(4)));

#define TB_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0)

static __device__ __attribute__((aligned(256))) float g_tokb_zero[64];     // stays zero: source of staged rows beyond the window

// x = a + b + c exactly (8 + 8 + 8 significand bits).  x is pinned to ONE rounded fp32 value first (tokens.hip's
// tk_split: with the producer's arithmetic visible the high piece and the residual must see the same value).
__device__ __forceinline__ void tb_split(float x, __bf16& a, __bf16& b, __bf16& c)
{
    asm volatile("" : "+v"(x));
    a = (__bf16)x;
    const float r1 = x - (float)a;
    b = (__bf16)r1;
    const float r2 = r1 - (float)b;
    c = (__bf16)r2;
}
struct TbOp {
    tb_bf16x8 p[3];         // hi, mid, lo
};
__device__ __forceinline__ void tb_split8(const float (&v)[8], TbOp& o)
{
#pragma unroll
    for (int e = 0; e < 8; ++e) { __bf16 a, b, c; tb_split(v[e], a, b, c); o.p[0][e] = a; o.p[1][e] = b; o.p[2][e] = c; }
}
// acc += A B over one 16-channel step: the six products, smallest first
__device__ __forceinline__ void tb_mac6(const TbOp& a, const TbOp& b, f32x16& acc)
{
    acc = TB_MFMA(a.p[2], b.p[0], acc);
    acc = TB_MFMA(a.p[1], b.p[1], acc);
    acc = TB_MFMA(a.p[0], b.p[2], acc);
    acc = TB_MFMA(a.p[1], b.p[0], acc);
    acc = TB_MFMA(a.p[0], b.p[1], acc);
    acc = TB_MFMA(a.p[0], b.p[0], acc);
}

// ------------------------------------------------------------------ token GEMM, bf16x6
#define TB_BM 128
#define TB_BN 128
#define TB_BK 16
#define TB_LDB 48          // bytes per LDS row: 16 bf16 (32 B) + 16 B pad (conflict-free b128 reads)

struct TokGemm6Params {
    const float* a;         // [M][K] f32 rows
    const __bf16* wgt;      // [3][N][K] bf16 planes (hi, mid, lo)
    const float* scale;     // [N] or null (a folded BatchNorm)
    const float* bias;      // [N] or null
    const float* residual;  // [*][ldr] f32, indexed by OUTPUT row, or null
    const int* rowmap;      // [M] output row of GEMM row m (-1: dropped) or null
    float* out;             // [*][ldc]
    int M, K, N, ldc, ldr, act;
    int64_t plane;          // elements per weight plane = N * K
};

// Tile 128 rows x 128 columns x 16 channels per step, four waves of 64 x 64, double-buffered LDS: staging, fragment
// reads and product order of conv2d_bf16x6_kernel with a pixel = a row.  Each output element is read (residual) and
// written by one lane, so `residual` may be `out`.
__global__ __launch_bounds__(256, 2) void tok_linear_bf16x6_kernel(TokGemm6Params p)
{
    __shared__ __attribute__((aligned(16))) unsigned char lds[2][2][3][TB_BM * TB_LDB];    // [buf][A|B][plane][row * 48 B]
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int wm = wave & 1, wn = wave >> 1;
    const int m0 = blockIdx.x * TB_BM, n0 = blockIdx.y * TB_BN;

    // A staging: 128 rows x 16 ch f32 = 4 float4 per row -> 512 float4, 2 per thread
    const int aq = tid & 3, ar = tid >> 2;            // piece, row (0..63), +64 on pass 1
    // B staging: per plane 128 rows x 16 bf16 = 2 x 16 B per row -> 256 pieces, 1 per thread
    const int bq = tid & 1, br = tid >> 1;
    const int nsteps = p.K / TB_BK;

    float4 ra[2];
    uint4 rb[3];
    auto load_step = [&](int step) {
        const int c0 = step * TB_BK;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int m = m0 + ar + 64 * i;
            ra[i] = m < p.M ? *reinterpret_cast<const float4*>(p.a + (int64_t)m * p.K + c0 + 4 * aq)
                            : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        const int n = n0 + br;
#pragma unroll
        for (int pl = 0; pl < 3; ++pl)
            rb[pl] = n < p.N ? *reinterpret_cast<const uint4*>(p.wgt + pl * p.plane + (int64_t)n * p.K + c0 + 8 * bq)
                             : make_uint4(0u, 0u, 0u, 0u);
    };
    auto store_step = [&](int buf) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const float v[4] = {ra[i].x, ra[i].y, ra[i].z, ra[i].w};
            tb_bf16x4 h, m, l;
#pragma unroll
            for (int e = 0; e < 4; ++e) { __bf16 a, bb, c; tb_split(v[e], a, bb, c); h[e] = a; m[e] = bb; l[e] = c; }
            const int off = (ar + 64 * i) * TB_LDB + 8 * aq;
            *reinterpret_cast<tb_bf16x4*>(&lds[buf][0][0][off]) = h;
            *reinterpret_cast<tb_bf16x4*>(&lds[buf][0][1][off]) = m;
            *reinterpret_cast<tb_bf16x4*>(&lds[buf][0][2][off]) = l;
        }
#pragma unroll
        for (int pl = 0; pl < 3; ++pl)
            *reinterpret_cast<uint4*>(&lds[buf][1][pl][br * TB_LDB + 16 * bq]) = rb[pl];
    };

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    load_step(0);
    store_step(0);
    __syncthreads();
    const int fr = lane & 31, fh = lane >> 5;
    for (int step = 0; step < nsteps; ++step) {
        const int buf = step & 1;
        if (step + 1 < nsteps) load_step(step + 1);
        TbOp a[2], b[2];
#pragma unroll
        for (int pl = 0; pl < 3; ++pl)
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                a[t].p[pl] = *reinterpret_cast<const tb_bf16x8*>(&lds[buf][0][pl][(wm * 64 + t * 32 + fr) * TB_LDB + 16 * fh]);
                b[t].p[pl] = *reinterpret_cast<const tb_bf16x8*>(&lds[buf][1][pl][(wn * 64 + t * 32 + fr) * TB_LDB + 16 * fh]);
            }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) tb_mac6(a[i], b[j], acc[i][j]);
        if (step + 1 < nsteps) store_step(buf ^ 1);
        __syncthreads();
    }

    // C layout: column = fr, rows (r & 3) + 8 (r >> 2) + 4 fh down the registers
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = m0 + wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * fh;
            if (m >= p.M) continue;
            const int orow = p.rowmap ? p.rowmap[m] : m;
            if (orow < 0) continue;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int n = n0 + wn * 64 + j * 32 + fr;
                if (n >= p.N) continue;
                float v = acc[i][j][r];
                if (p.scale) v = v * p.scale[n];
                if (p.bias) v = v + p.bias[n];
                if (p.act == 1) v = tk_gelu(v);
                else if (p.act == 2) v = v <= 0.f ? 0.f : v;         // NaN propagates, like torch.relu
                if (p.residual) v += p.residual[(int64_t)orow * p.ldr + n];
                p.out[(int64_t)orow * p.ldc + n] = v;
            }
        }
    }
}

extern "C" int al3d_tok_linear_bf16x6(const float* a, const void* wgt_bf16x3, const float* scale, const float* bias,
                                      int64_t M, int K, int N, int act, const float* residual, int ldr,
                                      const int* rowmap, float* out, int ldc, void* stream)
{
    AL3D_REQUIRE(a && wgt_bf16x3 && out, "al3d_tok_linear_bf16x6: null pointer");
    AL3D_REQUIRE(M >= 0 && M < ((int64_t)1 << 31) - 128 && K >= 16 && K % 16 == 0 && N >= 1, "al3d_tok_linear_bf16x6: bad shape M=%lld K=%d N=%d",
                 (long long)M, K, N);
    AL3D_REQUIRE(N % 4 == 0 && ldc % 4 == 0 && ldc >= N, "al3d_tok_linear_bf16x6: N=%d, ldc=%d must be multiples of 4, ldc >= N", N, ldc);
    AL3D_REQUIRE(!residual || (ldr % 4 == 0 && ldr >= N), "al3d_tok_linear_bf16x6: ldr=%d must be a multiple of 4 and >= N", ldr);
    AL3D_REQUIRE(act >= 0 && act <= 2, "al3d_tok_linear_bf16x6: act = 0 (none), 1 (GELU) or 2 (ReLU)");
    AL3D_REQUIRE((((uintptr_t)a | (uintptr_t)wgt_bf16x3 | (uintptr_t)out | (uintptr_t)residual) & 15) == 0,
                 "al3d_tok_linear_bf16x6: a / wgt / out / residual must be 16-byte aligned");
    AL3D_REQUIRE(al3d_cdiv(N, TB_BN) <= 65535, "al3d_tok_linear_bf16x6: N=%d needs more than 65535 column blocks", N);
    if (M == 0) return AL3D_OK;
    TokGemm6Params p;
    p.a = a; p.wgt = (const __bf16*)wgt_bf16x3; p.scale = scale; p.bias = bias; p.residual = residual; p.rowmap = rowmap;
    p.out = out; p.M = (int)M; p.K = K; p.N = N; p.ldc = ldc; p.ldr = ldr; p.act = act;
    p.plane = (int64_t)N * K;
    const dim3 grid((unsigned)al3d_cdiv(M, TB_BM), (unsigned)al3d_cdiv(N, TB_BN));
    hipLaunchKernelGGL(tok_linear_bf16x6_kernel, grid, dim3(256), 0, (hipStream_t)stream, p);
    AL3D_CHECK_LAUNCH("tok_linear_bf16x6_kernel");
    return AL3D_OK;
}

// ------------------------------------------------------------------ 7 x 7 window attention, head dim 32, bf16x6
// tok_window_attention_kernel with the bf16 split: two waves per (window, head), one 32-query tile each; the head's q, k,
// v rows staged as f32 by LDS-DMA with the same source-side chunk permutation; S^T = K (Q scale)^T with the keys on the
// accumulator rows, relative position bias + region mask + softmax down the registers in fp32, O^T = V^T P^T with P taken
// from the accumulators as the B operand.  Each product is six bf16 MFMAs into one accumulator.
__global__ __launch_bounds__(128, 2) void tok_window_attention_bf16x6_kernel(TokAttnParams p)
{
    __shared__ __attribute__((aligned(1024))) unsigned char stg[3 * TK_ABYTES];    // k | q | v
    __shared__ float tbl[176];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const int item = blockIdx.x;
    const int win = item / p.heads, head = item - win * p.heads;
    const int c = lane & 31, h = lane >> 5;
    const int ld = 3 * p.C;
    const float* base = p.qkv + (int64_t)win * TK_NT * ld + head * 32;
    const unsigned stg_base = (unsigned)(size_t)(tk_lds_void*)stg;
    const int wi = win % (p.nwy * p.nwx), wb = win / (p.nwy * p.nwx), wy = wi / p.nwx, wx = wi - wy * p.nwx;
    // token-order mode: token row of window position `row`, -1 for padding (shifted[hp] = padded[(hp + shift) % Hp])
    auto token_of = [&](int row) __attribute__((always_inline)) -> int {
        const int ty = (row * 37) >> 8, tx = row - ty * TK_WS;
        int hs = wy * TK_WS + ty + p.shift, ws = wx * TK_WS + tx + p.shift;
        hs -= hs >= p.nwy * TK_WS ? p.nwy * TK_WS : 0;
        ws -= ws >= p.nwx * TK_WS ? p.nwx * TK_WS : 0;
        return hs < p.H && ws < p.W ? (wb * p.H + hs) * p.W + ws : -1;
    };
    {
        const int rl = lane >> 3, pos = lane & 7;
#pragma unroll
        for (int it0 = 0; it0 < 4; ++it0) {
            const int it = 2 * it0 + wave;                      // the row groups of an array alternate between the waves
            if (it >= 7) continue;
            const int row = it * 8 + rl;
            const int chunk = pos ^ ((row >> 1) & 7);
            const bool live = row < TK_NT;
            const float* rp = g_tokb_zero;
            if (live) {
                rp = base + (int64_t)row * ld;
                if (p.bias) {
                    const int tok = token_of(row);
                    rp = (tok >= 0 ? p.qkv + (int64_t)tok * ld : p.bias) + head * 32;
                }
            }
            rp += chunk * 4;
#pragma unroll
            for (int arr = 0; arr < 3; ++arr) {
                const int aoff = live ? (arr == 0 ? p.C : arr == 1 ? 0 : 2 * p.C) : 0;
                const unsigned dst = __builtin_amdgcn_readfirstlane(stg_base + arr * TK_ABYTES + it * 1024);
                __builtin_amdgcn_global_load_lds((tk_gbl_void*)(rp + aoff), (tk_lds_void*)(size_t)dst, 16, 0, 0);
            }
        }
    }
    float tv[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) { const int t = threadIdx.x + 128 * k; tv[k] = t < 169 ? p.table[t * p.heads + head] : 0.f; }
    // shifted-window regions of the window's 7 rows / 7 columns, two bits each (uniform): tokens attend inside a region
    int rycode = 0, rxcode = 0;
    if (p.shift > 0) {
        for (int t = 0; t < TK_WS; ++t) {
            rycode |= tk_region1(wy * TK_WS + t, p.nwy * TK_WS, p.shift) << (2 * t);
            rxcode |= tk_region1(wx * TK_WS + t, p.nwx * TK_WS, p.shift) << (2 * t);
        }
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) { const int t = threadIdx.x + 128 * k; if (t < 176) tbl[t] = tv[k]; }
    tk_wait_vm<0>();
    __syncthreads();                                   // both waves' shares of k, q and v have landed
    __builtin_amdgcn_s_waitcnt(0xc07f);
    __builtin_amdgcn_wave_barrier();
    asm volatile("" ::: "memory");                     // the staged rows were written by the DMA, not by a store the compiler saw

    const bool masked = p.shift > 0;
    const float* stgf = reinterpret_cast<const float*>(stg);
    auto frag = [&](int arr, int row, int s, TbOp& o, float mul) __attribute__((always_inline)) {
        // channels 16 s + 8 h .. + 7 of staged row `row` of array arr (0 k, 1 q, 2 v)
        const float4 lo = *reinterpret_cast<const float4*>(stgf + ((arr * TK_ABYTES + tk_arow_off(row, 4 * s + 2 * h)) >> 2));
        const float4 hi = *reinterpret_cast<const float4*>(stgf + ((arr * TK_ABYTES + tk_arow_off(row, 4 * s + 2 * h + 1)) >> 2));
        const float v[8] = {lo.x * mul, lo.y * mul, lo.z * mul, lo.w * mul, hi.x * mul, hi.y * mul, hi.z * mul, hi.w * mul};
        tb_split8(v, o);
    };
    {
        const int query = 32 * wave + c;                   // this wave's query tile
        TbOp q[2];
#pragma unroll
        for (int s = 0; s < 2; ++s) frag(1, query, s, q[s], p.scale);
        f32x16 sm[2];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) sm[i][r] = 0.f;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                TbOp k;                                     // K fragment (A operand: rows = keys), split here
                frag(0, 32 * i + c, s, k, 1.0f);
                tb_mac6(k, q[s], sm[i]);
            }
        // logits -> probabilities, in place in sm[i] (rows = keys, column = this lane's query)
        const int qq = query < TK_NT ? query : TK_NT - 1;
        const int qy = (qq * 37) >> 8, qx = qq - TK_WS * qy;
        const int qcode = qq + 6 * qy + 84;                          // 13 y + x + 84
        // bit k of `diff`: key k lies in ANOTHER shifted-window region than this query (-100 on its logit)
        unsigned dlo = 0u, dhi = 0u;
        if (masked) {
            const int myry = (rycode >> (2 * qy)) & 3, myrx = (rxcode >> (2 * qx)) & 3;
            unsigned colmask = 0u;
            unsigned long long same = 0ull;
#pragma unroll
            for (int t = 0; t < TK_WS; ++t) colmask |= (unsigned)(((rxcode >> (2 * t)) & 3) == myrx) << t;
#pragma unroll
            for (int t = 0; t < TK_WS; ++t)
                if (((rycode >> (2 * t)) & 3) == myry) same |= (unsigned long long)colmask << (TK_WS * t);
            const unsigned long long diff = ~same >> (4 * h);        // the lane's keys are c + 4 h with compile-time c
            dlo = (unsigned)diff;
            dhi = (unsigned)(diff >> 32);
        }
        const float* tq = tbl + qcode;
        float mx = -INFINITY;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int cc = 32 * i + (r & 3) + 8 * (r >> 2);      // key = cc + 4 h
                float v = sm[i][r] + tq[-(h ? tk_kcode(cc + 4) : tk_kcode(cc))];
                if (masked) v += (float)(((cc < 32 ? dlo : dhi) >> (cc & 31)) & 1u) * -100.0f;
                if (cc + 4 >= TK_NT) v = (cc >= TK_NT || h) ? -INFINITY : v;
                sm[i][r] = v;
                mx = fmaxf(mx, v);
            }
        }
        mx = fmaxf(mx, __shfl_xor(mx, 32));
        float sum = 0.f;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                // e^(v - mx) = 2^((v - mx) log2 e): the product in two pieces, as in tok_window_attention_kernel
                const float d = sm[i][r] - mx;
                const float t = __builtin_fmaf(d, 1.44269502162933349609f, d * 1.92596299112661746e-8f);
                const float e = __builtin_amdgcn_exp2f(t);
                sm[i][r] = e;
                sum += e;
            }
        sum += __shfl_xor(sum, 32);
        const float inv = 1.0f / sum;
        // O^T[d][query] = sum_key V[key][d] P[query][key]; P is normalised AFTER the product (one multiply per output)
        f32x16 om;
#pragma unroll
        for (int r = 0; r < 16; ++r) om[r] = 0.f;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                float vv[8], pv[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const int key = 32 * i + 16 * s + 8 * (e >> 2) + 4 * h + (e & 3);
                    vv[e] = stgf[((2 * TK_ABYTES + tk_arow_off(key, c >> 2)) >> 2) + (c & 3)];
                    pv[e] = sm[i][8 * s + e];
                }
                TbOp v, pr;
                tb_split8(vv, v);
                tb_split8(pv, pr);
                tb_mac6(v, pr, om);
            }
        if (query >= TK_NT) return;
        // rows of O^T are d = (r & 3) + 8 (r >> 2) + 4 h: four consecutive channels per register quad
        int64_t out_row = (int64_t)win * TK_NT + query;
        if (p.bias) {
            out_row = token_of(query);
            if (out_row < 0) return;                         // a padded position's output is cropped
        }
        float* orow = p.out + out_row * p.C + head * 32;
#pragma unroll
        for (int g = 0; g < 4; ++g)
            *reinterpret_cast<float4*>(orow + 8 * g + 4 * h) =
                make_float4(om[4 * g] * inv, om[4 * g + 1] * inv, om[4 * g + 2] * inv, om[4 * g + 3] * inv);
    }
}

extern "C" int al3d_tok_window_attention_bf16x6(const float* qkv, const float* table, int nwin, int C, int heads,
                                                int win_rows, int win_cols, int shift, float scale, float* out,
                                                void* stream)
{
    AL3D_REQUIRE(qkv && table && out, "al3d_tok_window_attention_bf16x6: null pointer");
    AL3D_REQUIRE(nwin >= 0 && heads >= 1 && C == heads * 32, "al3d_tok_window_attention_bf16x6: C=%d must be heads (%d) x 32", C, heads);
    AL3D_REQUIRE(win_rows >= 1 && win_cols >= 1 && nwin % (win_rows * win_cols) == 0,
                 "al3d_tok_window_attention_bf16x6: nwin=%d is not a whole number of %d x %d window grids", nwin, win_rows, win_cols);
    AL3D_REQUIRE(shift >= 0 && shift < TK_WS, "al3d_tok_window_attention_bf16x6: shift=%d outside [0, 7)", shift);
    AL3D_REQUIRE((((uintptr_t)qkv | (uintptr_t)out) & 15) == 0, "al3d_tok_window_attention_bf16x6: qkv / out must be 16-byte aligned");
    if (nwin == 0) return AL3D_OK;
    const int64_t items = (int64_t)nwin * heads;
    AL3D_REQUIRE(items < ((int64_t)1 << 31), "al3d_tok_window_attention_bf16x6: too many (window, head) items");
    TokAttnParams p{qkv, table, out, nwin, C, heads, win_rows, win_cols, shift, scale, 0, nullptr, 0, 0};
    hipLaunchKernelGGL(tok_window_attention_bf16x6_kernel, dim3((unsigned)items), dim3(128), 0, (hipStream_t)stream, p);
    AL3D_CHECK_LAUNCH("tok_window_attention_bf16x6_kernel");
    return AL3D_OK;
}

extern "C" int al3d_tok_window_attention_tokens_bf16x6(const float* qkv, const float* bias_qkv, const float* table, int B,
                                                       int H, int W, int C, int heads, int shift, float scale,
                                                       float* out, void* stream)
{
    AL3D_REQUIRE(B >= 0 && H >= 1 && W >= 1 && (int64_t)B * H * W < ((int64_t)1 << 31), "al3d_tok_window_attention_tokens_bf16x6: bad map size");
    if (B == 0) return AL3D_OK;
    AL3D_REQUIRE(qkv && bias_qkv && table && out, "al3d_tok_window_attention_tokens_bf16x6: null pointer (a model without qkv bias passes zeros)");
    AL3D_REQUIRE(heads >= 1 && C == heads * 32, "al3d_tok_window_attention_tokens_bf16x6: C=%d must be heads (%d) x 32", C, heads);
    AL3D_REQUIRE(shift >= 0 && shift < TK_WS, "al3d_tok_window_attention_tokens_bf16x6: shift=%d outside [0, 7)", shift);
    AL3D_REQUIRE((((uintptr_t)qkv | (uintptr_t)out | (uintptr_t)bias_qkv) & 15) == 0, "al3d_tok_window_attention_tokens_bf16x6: qkv / bias / out must be 16-byte aligned");
    const int nwy = (H + TK_WS - 1) / TK_WS, nwx = (W + TK_WS - 1) / TK_WS;
    const int64_t items = (int64_t)B * nwy * nwx * heads;
    AL3D_REQUIRE(items < ((int64_t)1 << 31), "al3d_tok_window_attention_tokens_bf16x6: too many (window, head) items");
    TokAttnParams p{qkv, table, out, B * nwy * nwx, C, heads, nwy, nwx, shift, scale, 0, bias_qkv, H, W};
    hipLaunchKernelGGL(tok_window_attention_bf16x6_kernel, dim3((unsigned)items), dim3(128), 0, (hipStream_t)stream, p);
    AL3D_CHECK_LAUNCH("tok_window_attention_bf16x6_kernel");
    return AL3D_OK;
}

// ------------------------------------------------------------------ multi-head attention, head dim 16, bf16x6
// tok_mha16_kernel with the bf16 split: one wave per (sample, head, 32-query tile, key chunk), online softmax down the
// accumulator registers, (max, sum, O[16]) per chunk, merged by tok_mha16_combine_kernel (tok_shared.h).
__global__ __launch_bounds__(64) void tok_mha16_bf16x6_kernel(TokMhaParams p)
{
    const int lane = threadIdx.x, c = lane & 31, h = lane >> 5;
    int id = blockIdx.x;
    const int chunk = id % p.chunks; id /= p.chunks;
    const int qt = id % p.qtiles; id /= p.qtiles;
    const int head = id % p.heads;
    const int b = id / p.heads;
    const int query = qt * 32 + c;
    TbOp q;
    {
        float qv[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (query < p.Pq) {
            const float* qp = p.q + ((int64_t)b * p.Pq + query) * p.ldq + head * 16 + 8 * h;
            const float4 a = *reinterpret_cast<const float4*>(qp), b4 = *reinterpret_cast<const float4*>(qp + 4);
            qv[0] = a.x * p.scale; qv[1] = a.y * p.scale; qv[2] = a.z * p.scale; qv[3] = a.w * p.scale;
            qv[4] = b4.x * p.scale; qv[5] = b4.y * p.scale; qv[6] = b4.z * p.scale; qv[7] = b4.w * p.scale;
        }
        tb_split8(qv, q);
    }
    const int key0 = chunk * p.keys_per_chunk;
    const int key1 = key0 + p.keys_per_chunk < p.Pk ? key0 + p.keys_per_chunk : p.Pk;
    const float* kb = p.k + (int64_t)b * p.Pk * p.ldk + head * 16;
    const float* vb = p.v + (int64_t)b * p.Pk * p.ldv + head * 16;
    float run_max = -INFINITY, run_sum = 0.f;
    f32x16 om;
#pragma unroll
    for (int r = 0; r < 16; ++r) om[r] = 0.f;
    for (int kt = key0; kt < key1; kt += 32) {
        // K tile: A operand, lane (key c, half h) holds K[key][8 h .. 8 h + 7]
        TbOp k;
        {
            float kv[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            if (kt + c < key1) {
                const float* kp = kb + (int64_t)(kt + c) * p.ldk + 8 * h;
                const float4 a = *reinterpret_cast<const float4*>(kp), b4 = *reinterpret_cast<const float4*>(kp + 4);
                kv[0] = a.x; kv[1] = a.y; kv[2] = a.z; kv[3] = a.w; kv[4] = b4.x; kv[5] = b4.y; kv[6] = b4.z; kv[7] = b4.w;
            }
            tb_split8(kv, k);
        }
        // V^T fragments of the tile's two k-steps (issued early: their latency hides behind the logits)
        float vv[2][8];
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int key = kt + 16 * s + 8 * (e >> 2) + 4 * h + (e & 3);
                vv[s][e] = (c < 16 && key < key1) ? vb[(int64_t)key * p.ldv + c] : 0.f;
            }
        f32x16 sm;
#pragma unroll
        for (int r = 0; r < 16; ++r) sm[r] = 0.f;
        tb_mac6(k, q, sm);
        float mx = run_max;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int key = kt + (r & 3) + 8 * (r >> 2) + 4 * h;
            const float v = key < key1 ? sm[r] : -INFINITY;
            sm[r] = v;
            mx = fmaxf(mx, v);
        }
        mx = fmaxf(mx, __shfl_xor(mx, 32));              // every tile holds at least one real key: mx is finite
        const float resc = __builtin_amdgcn_exp2f((run_max - mx) * 1.44269504088896340736f);     // 0 on the first tile
        float sum = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float d = sm[r] - mx;
            const float e = __builtin_amdgcn_exp2f(__builtin_fmaf(d, 1.44269502162933349609f, d * 1.92596299112661746e-8f));
            sm[r] = e;
            sum += e;
        }
        sum += __shfl_xor(sum, 32);
        run_sum = run_sum * resc + sum;
        run_max = mx;
#pragma unroll
        for (int r = 0; r < 16; ++r) om[r] *= resc;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            float pv[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) pv[e] = sm[8 * s + e];
            TbOp v, pr;
            tb_split8(vv[s], v);
            tb_split8(pv, pr);
            tb_mac6(v, pr, om);
        }
    }
    // rows of O^T: d = (r & 3) + 8 (r >> 2) + 4 h; d < 16 <=> r < 8
    float* o = p.part + ((((int64_t)b * p.heads + head) * p.chunks + chunk) * (p.qtiles * 32) + query) * 18;
    if (h == 0) { o[0] = run_max; o[1] = run_sum; }
#pragma unroll
    for (int r = 0; r < 8; ++r) o[2 + (r & 3) + 8 * (r >> 2) + 4 * h] = om[r];
}

extern "C" int al3d_tok_mha16_bf16x6(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, int B,
                                     int heads, int Pq, int Pk, float scale, float* out, int ldo, void* workspace,
                                     void* stream)
{
    AL3D_REQUIRE(q && k && v && out && workspace, "al3d_tok_mha16_bf16x6: null pointer");
    AL3D_REQUIRE(B >= 1 && heads >= 1 && Pq >= 1 && Pk >= 1, "al3d_tok_mha16_bf16x6: bad shape");
    AL3D_REQUIRE(ldq >= heads * 16 && ldk >= heads * 16 && ldv >= heads * 16 && ldo >= heads * 16 && ldq % 4 == 0 && ldk % 4 == 0,
                 "al3d_tok_mha16_bf16x6: row pitches must cover heads x 16 channels (q, k pitches multiples of 4)");
    AL3D_REQUIRE((((uintptr_t)q | (uintptr_t)k) & 15) == 0, "al3d_tok_mha16_bf16x6: q / k must be 16-byte aligned");
    TokMhaParams p;
    p.q = q; p.k = k; p.v = v; p.part = (float*)workspace;
    p.B = B; p.heads = heads; p.Pq = Pq; p.Pk = Pk; p.ldq = ldq; p.ldk = ldk; p.ldv = ldv;
    p.qtiles = (Pq + 31) / 32;
    p.chunks = (Pk + 1023) / 1024;
    p.keys_per_chunk = (int)al3d_align(al3d_cdiv(Pk, p.chunks), 32);
    p.chunks = (int)al3d_cdiv(Pk, p.keys_per_chunk);       // no empty chunk: every partial holds at least one key
    p.scale = scale;
    const int64_t waves = (int64_t)B * heads * p.qtiles * p.chunks;
    AL3D_REQUIRE(waves < ((int64_t)1 << 31), "al3d_tok_mha16_bf16x6: too many work items");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(tok_mha16_bf16x6_kernel, dim3((unsigned)waves), dim3(64), 0, s, p);
    AL3D_CHECK_LAUNCH("tok_mha16_bf16x6_kernel");
    const int64_t n = (int64_t)B * heads * Pq * 16;
    hipLaunchKernelGGL(tok_mha16_combine_kernel, dim3((unsigned)al3d_cdiv(n, 256)), dim3(256), 0, s, (const float*)workspace, B,
                       heads, p.chunks, p.qtiles * 32, Pq, out, ldo);
    AL3D_CHECK_LAUNCH("tok_mha16_combine_kernel");
    return AL3D_OK;
}
