// Token-matrix kernels in fp32-faithful bf16x6 arithmetic (AL3D_MATH=bf16x6 / f32 on the token path): the token GEMM,
// the 7 x 7 window attention (both row orders) and the head-dim-16 attention of tokens.hip with every matrix product
// formed by al3d_bf16x6.h's rule (three-way exact split, six products into ONE accumulator).  The bf16 product has the
// fragment shapes of the f16 one, so the two attention kernels are tok_attention.h's templates -- the code tokens.hip
// runs -- instantiated for this file's arithmetic TkBf16x6.  f32 rows in and out: pair rows are f16 planes and do not
// exist here.
//
//   tok_linear_bf16x6_kernel               al3d_bf16x6.h's 128 x 128 x 16 tile pipeline on token rows; activations
//                                          split while they are staged, weights pre-split [3][N][K]; epilogue: scale,
//                                          bias, exact GELU / ReLU, residual, row scatter
//   tok_window_attention_kernel<TkBf16x6>  q (scaled), k, v and the probabilities split three ways; softmax in fp32 VALU
//   tok_mha16_kernel<TkBf16x6>             the same for 16-channel heads, chunked online softmax, + the shared combine
//
// Written for correctness over the full fp32 range, not for speed.  gfx950 only.
#include "al3d_common.h"
#include "al3d_bf16x6.h"
#include "tok_attention.h"

// The shared split of a value PINNED to one rounded fp32 value first (al3d_f16x3.h's f3_split_pinned: with the producer's
// arithmetic visible the high piece and the residual must see the same value).
__device__ __forceinline__ void tb_split(float x, __bf16& a, __bf16& b, __bf16& c)
{
    asm volatile("" : "+v"(x));
    b6_split(x, a, b, c);
}
__device__ __forceinline__ void tb_split8(const float (&v)[8], B6Frag& o)
{
#pragma unroll
    for (int e = 0; e < 8; ++e) { __bf16 a, b, c; tb_split(v[e], a, b, c); o.p[0][e] = a; o.p[1][e] = b; o.p[2][e] = c; }
}

// ------------------------------------------------------------------ token GEMM, bf16x6
#define TB_BM 128
#define TB_BN 128

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

// al3d_bf16x6.h's tile pipeline: A rows = token rows, B rows = output columns; staged values go through the pinned
// split like every other token operand.  Each output element is read (residual) and written by one lane, so `residual`
// may be `out`.
__global__ __launch_bounds__(256, 2) void tok_linear_bf16x6_kernel(TokGemm6Params p)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm = wave & 1, wn = wave >> 1;
    const int m0 = blockIdx.x * TB_BM, n0 = blockIdx.y * TB_BN;

    auto load_a = [&](int step, int row, int q, float4 (&ra)[2]) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int m = m0 + row + 64 * i;
            ra[i] = m < p.M ? *reinterpret_cast<const float4*>(p.a + (int64_t)m * p.K + step * 16 + 4 * q)
                            : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };
    auto load_b = [&](int step, int row, int q, uint4 (&rb)[3]) {
        const int n = n0 + row;
#pragma unroll
        for (int pl = 0; pl < 3; ++pl)
            rb[pl] = n < p.N ? *reinterpret_cast<const uint4*>(p.wgt + pl * p.plane + (int64_t)n * p.K + step * 16 + 8 * q)
                             : make_uint4(0u, 0u, 0u, 0u);
    };
    f32x16 acc[2][2];
    b6_tile_pipeline<tb_split>(p.K / 16, load_a, load_b, acc);

    const int fr = lane & 31, fh = lane >> 5;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = m0 + wm * 64 + i * 32 + b6_crow(r, fh);
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

// ------------------------------------------------------------------ window attention and head-dim-16 attention (tok_attention.h)
// q (scaled), k, v and the probabilities split three ways; each product is six bf16 MFMAs into one accumulator.  f32 rows
// out: pair rows are f16 planes and do not exist here.
struct TkBf16x6 {
    using Frag = B6Frag;
    using Acc = f32x16;
    static constexpr int kWavesPerSimd = 2;
    static constexpr bool kPairRows = false;
    static __device__ __forceinline__ void split8(float (&v)[8], Frag& o) { tb_split8(v, o); }
    static __device__ __forceinline__ void mac(const Frag& a, const Frag& b, Acc& acc) { b6_mac6(a, b, acc); }
    static __device__ __forceinline__ float value(const Acc& a, int r) { return a[r]; }
    static __device__ __forceinline__ void rescale(Acc& a, float f) { a *= f; }
};
template __global__ void tok_window_attention_kernel<TkBf16x6>(TokAttnParams);
template __global__ void tok_mha16_kernel<TkBf16x6>(TokMhaParams);

extern "C" int al3d_tok_window_attention_bf16x6(const float* qkv, const float* table, int nwin, int C, int heads,
                                                int win_rows, int win_cols, int shift, float scale, float* out,
                                                void* stream)
{
    const TokAttnParams p{qkv, table, out, nwin, C, heads, win_rows, win_cols, shift, scale, 0, nullptr, 0, 0};
    return tok_window_attention_launch<TkBf16x6>("al3d_tok_window_attention_bf16x6", false, 0, p, stream);
}

extern "C" int al3d_tok_window_attention_tokens_bf16x6(const float* qkv, const float* bias_qkv, const float* table, int B,
                                                       int H, int W, int C, int heads, int shift, float scale,
                                                       float* out, void* stream)
{
    const TokAttnParams p{qkv, table, out, 0, C, heads, 0, 0, shift, scale, 0, bias_qkv, H, W};
    return tok_window_attention_launch<TkBf16x6>("al3d_tok_window_attention_tokens_bf16x6", true, B, p, stream);
}

extern "C" int al3d_tok_mha16_bf16x6(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, int B,
                                     int heads, int Pq, int Pk, float scale, float* out, int ldo, void* workspace,
                                     void* stream)
{
    return tok_mha16_launch<TkBf16x6>("al3d_tok_mha16_bf16x6", q, ldq, k, ldk, v, ldv, B, heads, Pq, Pk, scale, out, ldo,
                                      workspace, stream);
}
