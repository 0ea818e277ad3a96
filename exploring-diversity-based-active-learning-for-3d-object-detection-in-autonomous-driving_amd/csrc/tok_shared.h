// Pieces shared by the token kernels of both arithmetics (tokens.hip: f16x3, tokens_bf16x6.hip: bf16x6) that do not
// depend on the operand format: the zero row, the erf / GELU of the GEMM epilogues, the parameter blocks
// and staged-row layout of the 7 x 7 window kernel, the head-dim-16 attention's parameter block and chunk combine kernel.
// The attention kernels themselves, with the window geometry and softmax, are in tok_attention.h.  The vector and
// address-space typedefs and the counted wait are al3d_f16x3.h's (they carry no arithmetic).
#pragma once
#include "al3d_common.h"
#include "al3d_f16x3.h"

static __device__ __attribute__((aligned(256))) float g_tok_zero[64];     // stays zero: source of rows beyond a matrix / window

// erf to fp32 rounding level, branch-free: the two minimax pieces of N. Juffa's single-precision erf (x + x P(x^2) below
// 475/512, 1 - exp(Q(|x|)) above; each < 1 ulp with an exact exp) are both evaluated and one is selected -- the library erff
// costs ~45 vector instructions and a divergent branch per element, and the GELU epilogues are bound by exactly that.
// exp through v_exp_f32 (2^x): its argument is <= -0.9, so the result is <= 0.41 and the error it adds to 1 - exp stays
// below 1e-7.  Measured against float64 over [-8, 8]: see tests/test_swin_gpu.py::test_gelu_epilogue_accuracy.
__device__ __forceinline__ float tk_erf(float a)
{
    const float t = fabsf(a), s = a * a;
    float r = __builtin_fmaf(-1.72853470e-5f, t, 3.83197126e-4f);
    const float u = __builtin_fmaf(-3.88396438e-3f, t, 2.42546219e-2f);
    r = __builtin_fmaf(r, s, u);
    r = __builtin_fmaf(r, t, -1.06777877e-1f);
    r = __builtin_fmaf(r, t, -6.34846687e-1f);
    r = __builtin_fmaf(r, t, -1.28717512e-1f);
    r = __builtin_fmaf(r, t, -t);
    float big = 1.0f - __builtin_amdgcn_exp2f(r * 1.44269504088896340736f);
    big = __builtin_copysignf(big, a);
    float q = -5.96761703e-4f;
    q = __builtin_fmaf(q, s, 4.99119423e-3f);
    q = __builtin_fmaf(q, s, -2.67681349e-2f);
    q = __builtin_fmaf(q, s, 1.12819925e-1f);
    q = __builtin_fmaf(q, s, -3.76125336e-1f);
    q = __builtin_fmaf(q, s, 1.28379166e-1f);
    q = __builtin_fmaf(q, a, a);
    return t > 0.927734375f ? big : q;
}

__device__ __forceinline__ float tk_gelu(float v)
{
    return (v * 0.5f) * (1.0f + tk_erf(v * 0.70710678118654752440f));
}

// ------------------------------------------------------------------ 7 x 7 window attention, head dim 32
struct TokAttnParams {
    const float* qkv;       // [nwin * 49][3 C]: q | k | v, each [heads][32]
    const float* table;     // [169][heads] relative position bias table
    float* out;             // [nwin * 49][C] f32 or pair rows
    int nwin, C, heads;
    int nwy, nwx;           // windows per image (rows, columns)
    int shift;              // cyclic shift of the block (0: no mask)
    float scale;
    int pair;
    // token-order mode (bias != null): qkv / out rows are the B maps' H x W tokens; the cyclic shift, the padding and the
    // window partition are evaluated from the window's position, a padded position's q / k / v row is the qkv bias
    const float* bias;      // [3 C] or null (window-order mode: rows win * 49 + position)
    int H, W;
};

#define TK_WS 7
#define TK_NT 49

__device__ __forceinline__ int tk_region1(int v, int n, int shift)
{
    return (v >= n - TK_WS ? 1 : 0) + (v >= n - shift ? 1 : 0);
}

// 13 y + x of key position min(key, 48) in the 7 x 7 window: the key's part of the relative position index
__host__ __device__ constexpr int tk_kcode(int key) { return (key < TK_NT ? key : TK_NT - 1) + 6 * ((key < TK_NT ? key : TK_NT - 1) / TK_WS); }

// staged q / k / v rows of one (window, head): see tok_window_attention_kernel
#define TK_AROWS 56                   // rows staged per array: 7 DMA instructions of 8 rows; rows 49 .. 55 are zero
#define TK_ABYTES (TK_AROWS * 128)

__device__ __forceinline__ unsigned tk_arow_off(int row, int chunk)      // byte offset of 16-byte chunk `chunk` of a staged row
{
    const int r = row < TK_AROWS ? row : TK_AROWS - 1;                   // rows 56 .. 63 of a tile read a zero row
    return (unsigned)(r * 128 + ((chunk ^ ((r >> 1) & 7)) << 4));
}

// ------------------------------------------------------------------ multi-head attention, head dim 16
struct TokMhaParams {
    const float* q;         // [B][Pq][ldq], this head's 16 channels at column head * 16
    const float* k;         // [B][Pk][ldk]
    const float* v;         // [B][Pk][ldv]
    float* part;            // [B][heads][chunks][qtiles * 32][18]: running max, sum, O[16]
    int B, heads, Pq, Pk, ldq, ldk, ldv;
    int qtiles, chunks, keys_per_chunk;          // keys_per_chunk: a multiple of 32
    float scale;
};

// out[b][query][head * 16 + d] = sum_c e^(m_c - M) O_c[d] / sum_c e^(m_c - M) l_c
static __global__ __launch_bounds__(256) void tok_mha16_combine_kernel(const float* __restrict__ part, int B, int heads, int chunks,
                                                                       int qrows, int Pq, float* __restrict__ out, int ldo)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (int64_t)B * heads * Pq * 16) return;
    const int d = (int)(t & 15);
    int64_t r = t >> 4;
    const int query = (int)(r % Pq); r /= Pq;
    const int head = (int)(r % heads);
    const int b = (int)(r / heads);
    const float* base = part + (((int64_t)b * heads + head) * chunks * qrows + query) * 18;
    float M = -INFINITY;
    for (int c = 0; c < chunks; ++c) M = fmaxf(M, base[(int64_t)c * qrows * 18]);
    float num = 0.f, den = 0.f;
    for (int c = 0; c < chunks; ++c) {
        const float* q = base + (int64_t)c * qrows * 18;
        const float w = expf(q[0] - M);
        num += w * q[2 + d];
        den += w * q[1];
    }
    out[((int64_t)b * Pq + query) * ldo + head * 16 + d] = num / den;
}
