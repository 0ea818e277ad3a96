// The two attention kernels of the token path, written once for both arithmetics, with the shifted-window geometry
// and softmax they share with the fused tok_attn_block_f16x3_kernel (tokens.hip), and their checked launchers.
//
// An arithmetic is a policy struct (TkF16x3 in tokens.hip, TkBf16x6 in tokens_bf16x6.hip):
//   Frag               the MFMA operand fragment of 8 fp32 values (all its planes)
//   split8(v, frag)    the split of 8 values into a fragment
//   Acc                the accumulator(s) of a 32 x 32 tile, `Acc a = {}` is zero
//   mac(a, b, acc)     acc += A B over one 16-channel step, in the arithmetic's product order
//   value(acc, r)      the fp32 value of accumulator register r
//   rescale(acc, f)    acc *= f (online softmax)
//   kWavesPerSimd      occupancy hint of the window kernel
//   kPairRows          pair rows (sp_rows.h) exist as an output; then store_pair4(dst, h, y) writes a lane's four
//
// tok_window_attention_kernel<Arith>   two waves (= one 128-thread workgroup) per (window, head), one 32-query tile each
// tok_mha16_kernel<Arith>              16-channel heads, any key count: one wave per (sample, head, 32-query tile, key
//                                      chunk), merged by tok_mha16_combine_kernel (tok_shared.h)
#pragma once
#include "tok_shared.h"

// ------------------------------------------------------------------ shifted-window geometry
struct TkWinPos { int b, y, x; };                       // sample, window row, window column

__device__ __forceinline__ TkWinPos tk_win_pos(int win, int nwy, int nwx)
{
    const int wi = win % (nwy * nwx), wy = wi / nwx;
    return {win / (nwy * nwx), wy, wi - wy * nwx};
}

// token row of window position `row` (< 85: (row * 37) >> 8 == row / 7) of an H x W map, -1 for padding:
// shifted[hp] = padded[(hp + shift) % Hp]
__device__ __forceinline__ int tk_token_of(int row, const TkWinPos& w, int nwy, int nwx, int shift, int H, int W)
{
    const int ty = (row * 37) >> 8, tx = row - ty * TK_WS;
    int hs = w.y * TK_WS + ty + shift, ws = w.x * TK_WS + tx + shift;
    hs -= hs >= nwy * TK_WS ? nwy * TK_WS : 0;
    ws -= ws >= nwx * TK_WS ? nwx * TK_WS : 0;
    return hs < H && ws < W ? (w.b * H + hs) * W + ws : -1;
}

// shifted-window regions of the window's 7 rows / 7 columns, two bits each (uniform): tokens attend inside a region
__device__ __forceinline__ void tk_region_codes(const TkWinPos& w, int nwy, int nwx, int shift, int& rycode, int& rxcode)
{
    rycode = 0; rxcode = 0;
    if (shift > 0) {
        for (int t = 0; t < TK_WS; ++t) {
            rycode |= tk_region1(w.y * TK_WS + t, nwy * TK_WS, shift) << (2 * t);
            rxcode |= tk_region1(w.x * TK_WS + t, nwx * TK_WS, shift) << (2 * t);
        }
    }
}

// bit k of (dhi:dlo): key k + 4 h lies in ANOTHER shifted-window region than the query at (qy, qx) (-100 on its logit).
// A bit mask per query instead of a region lookup per element: that form (an LDS read behind `if (masked)`) made hipcc
// serialise 64 LDS round trips per tile
__device__ __forceinline__ void tk_region_diff(int rycode, int rxcode, int qy, int qx, int h, unsigned& dlo, unsigned& dhi)
{
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

// e^d = 2^(d log2 e): the product in two pieces so that the argument of v_exp_f32 carries no rounding of its own beyond
// 2^-24 relative (|d| <= ~100 here)
__device__ __forceinline__ float tk_exp(float d)
{
    return __builtin_amdgcn_exp2f(__builtin_fmaf(d, 1.44269502162933349609f, d * 1.92596299112661746e-8f));
}

// logits -> unnormalised probabilities of one 32-query tile against the window's 64 key rows, in place; returns 1 / sum.
// sm[i] is a C tile of S^T: rows = keys (key = 32 i + (r & 3) + 8 (r >> 2) + 4 h down the registers), column = this
// lane's query.  + relative position bias (tbl: the head's 169 entries), -100 across shifted-window regions, -inf on
// the key rows 49 .. 63.
__device__ __forceinline__ float tk_window_softmax(f32x16 (&sm)[2], int query, int h, const float* tbl, bool masked,
                                                   int rycode, int rxcode)
{
    const int qq = query < TK_NT ? query : TK_NT - 1;
    const int qy = (qq * 37) >> 8, qx = qq - TK_WS * qy;
    const int qcode = qq + 6 * qy + 84;                          // 13 y + x + 84
    unsigned dlo = 0u, dhi = 0u;
    if (masked) tk_region_diff(rycode, rxcode, qy, qx, h, dlo, dhi);
    const float* tq = tbl + qcode;
    float mx = -INFINITY;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        float tb[16];                                            // the tile's 16 bias lookups first, then their uses
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int cc = 32 * i + (r & 3) + 8 * (r >> 2);      // key = cc + 4 h
            tb[r] = tq[-(h ? tk_kcode(cc + 4) : tk_kcode(cc))];
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int cc = 32 * i + (r & 3) + 8 * (r >> 2);
            float v = sm[i][r];
            v += tb[r];
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
            const float e = tk_exp(sm[i][r] - mx);
            sm[i][r] = e;
            sum += e;
        }
    sum += __shfl_xor(sum, 32);
    return 1.0f / sum;
}

// ------------------------------------------------------------------ 7 x 7 window attention, head dim 32
// channels 16 s + 8 h .. + 7 of staged row `row` of the array at LDS byte address `arr`.  The staged rows were written
// by the DMA, not by a store the compiler saw: they are read by instructions it cannot move or elide, and the wait
// belongs to the reads (separate asm statements could be scheduled apart from their uses)
__device__ __forceinline__ void tk_staged_row8(unsigned arr, int row, int s, int h, float (&v)[8])
{
    f32x4 lo, hi;
    asm volatile("ds_read_b128 %0, %2\n\tds_read_b128 %1, %3\n\ts_waitcnt lgkmcnt(0)"
                 : "=&v"(lo), "=&v"(hi)
                 : "v"(arr + tk_arow_off(row, 4 * s + 2 * h)), "v"(arr + tk_arow_off(row, 4 * s + 2 * h + 1))
                 : "memory");
#pragma unroll
    for (int e = 0; e < 4; ++e) { v[e] = lo[e]; v[4 + e] = hi[e]; }
}

// The head's q, k, v rows (49 x 128 B each, 1152+ B apart in the qkv matrix) come in by LDS-DMA, eight whole rows per
// instruction (every 128-byte line fetched once, by one instruction); a row's eight 16-byte chunks are stored permuted
// (chunk q at position q ^ ((row >> 1) & 7), applied on the SOURCE side: the LDS side of a DMA is lane-linear) so that
// the fragment reads are conflict-free.
// C-layout of v_mfma_f32_32x32x16: column = lane & 31, rows in the 16 registers
// (row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)); S^T = K (Q scale)^T puts the KEYS on the rows, so a query's softmax
// runs down a lane's registers (+ one exchange with lane ^ 32), and P^T is already the B operand of O^T = V^T P^T:
// registers 8 s .. 8 s + 7 of a tile are k-step s, in the order key = 16 s + 8 (j >> 2) + 4 h + (j & 3) -- the V^T
// fragment is read in that same order.  Both operands of both products are activations, split here.
// The two waves share the staged rows; K fragments are read (and split) where they are used instead of being held,
// and the state of a tile -- 64 logit + 32 output accumulators -- is all a wave keeps: that is what lets several waves
// share a SIMD (f16x3: six workgroups per CU by LDS, twelve resident waves).
template <class Arith>
__global__ __launch_bounds__(128, Arith::kWavesPerSimd) void tok_window_attention_kernel(TokAttnParams p)
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
    const unsigned stg_base = (unsigned)(size_t)(lds_void*)stg;
    const TkWinPos w = tk_win_pos(win, p.nwy, p.nwx);
    // the rows first (their latency is the longest: per row group ONE source row address serves the k, q and v pieces), then
    // the position-bias table and the region codes in its shadow -- with the table load in front every item began by
    // waiting for it before a single row was requested (35 % of an item's life by per-phase time stamps)
    {
        const int rl = lane >> 3, pos = lane & 7;
#pragma unroll
        for (int it0 = 0; it0 < 4; ++it0) {
            const int it = 2 * it0 + wave;                      // the row groups of an array alternate between the waves
            if (it >= 7) continue;
            const int row = it * 8 + rl;
            const int chunk = pos ^ ((row >> 1) & 7);
            const bool live = row < TK_NT;
            const float* rp = g_tok_zero;
            if (live) {
                rp = base + (int64_t)row * ld;
                if (p.bias) {                                   // token-order mode: a padded position reads the qkv bias
                    const int tok = tk_token_of(row, w, p.nwy, p.nwx, p.shift, p.H, p.W);
                    rp = (tok >= 0 ? p.qkv + (int64_t)tok * ld : p.bias) + head * 32;
                }
            }
            rp += chunk * 4;
#pragma unroll
            for (int arr = 0; arr < 3; ++arr) {
                const int aoff = live ? (arr == 0 ? p.C : arr == 1 ? 0 : 2 * p.C) : 0;
                const unsigned dst = __builtin_amdgcn_readfirstlane(stg_base + arr * TK_ABYTES + it * 1024);
                __builtin_amdgcn_global_load_lds((gbl_void*)(rp + aoff), (lds_void*)(size_t)dst, 16, 0, 0);
            }
        }
    }
    float tv[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) { const int t = threadIdx.x + 128 * k; tv[k] = t < 169 ? p.table[t * p.heads + head] : 0.f; }
    int rycode, rxcode;
    tk_region_codes(w, p.nwy, p.nwx, p.shift, rycode, rxcode);
#pragma unroll
    for (int k = 0; k < 2; ++k) { const int t = threadIdx.x + 128 * k; if (t < 176) tbl[t] = tv[k]; }
    f3_wait_vm<0>();
    __syncthreads();                                   // both waves' shares of k, q and v have landed
    __builtin_amdgcn_s_waitcnt(0xc07f);
    __builtin_amdgcn_wave_barrier();

    const int query = 32 * wave + c;                   // this wave's query tile
    typename Arith::Frag q[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        float qv[8];
        tk_staged_row8(stg_base + TK_ABYTES, query, s, h, qv);
#pragma unroll
        for (int e = 0; e < 8; ++e) qv[e] *= p.scale;
        Arith::split8(qv, q[s]);
    }
    typename Arith::Acc sa[2] = {};
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            float kv[8];                                     // K fragment (A operand: rows = keys), split here
            tk_staged_row8(stg_base, 32 * i + c, s, h, kv);
            typename Arith::Frag k;
            Arith::split8(kv, k);
            Arith::mac(k, q[s], sa[i]);
        }
    f32x16 sm[2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) sm[i][r] = Arith::value(sa[i], r);
    const float inv = tk_window_softmax(sm, query, h, tbl, p.shift > 0, rycode, rxcode);
    // O^T[d][query] = sum_key V[key][d] P[query][key]; P is normalised AFTER the product (one multiply per output)
    typename Arith::Acc oa = {};
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            float vv[8], pv[8];
            unsigned va[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int key = 32 * i + 16 * s + 8 * (e >> 2) + 4 * h + (e & 3);
                va[e] = stg_base + 2 * TK_ABYTES + tk_arow_off(key, c >> 2) + ((c & 3) << 2);
                pv[e] = sm[i][8 * s + e];
            }
            asm volatile("ds_read_b32 %0, %8\n\tds_read_b32 %1, %9\n\tds_read_b32 %2, %10\n\tds_read_b32 %3, %11\n\t"
                         "ds_read_b32 %4, %12\n\tds_read_b32 %5, %13\n\tds_read_b32 %6, %14\n\tds_read_b32 %7, %15\n\t"
                         "s_waitcnt lgkmcnt(0)"
                         : "=&v"(vv[0]), "=&v"(vv[1]), "=&v"(vv[2]), "=&v"(vv[3]), "=&v"(vv[4]), "=&v"(vv[5]), "=&v"(vv[6]), "=&v"(vv[7])
                         : "v"(va[0]), "v"(va[1]), "v"(va[2]), "v"(va[3]), "v"(va[4]), "v"(va[5]), "v"(va[6]), "v"(va[7])
                         : "memory");
            typename Arith::Frag v, pr;
            Arith::split8(vv, v);
            Arith::split8(pv, pr);
            Arith::mac(v, pr, oa);
        }
    if (query >= TK_NT) return;
    // rows of O^T are d = (r & 3) + 8 (r >> 2) + 4 h: four consecutive channels per register quad
    int64_t out_row = (int64_t)win * TK_NT + query;
    if (p.bias) {
        out_row = tk_token_of(query, w, p.nwy, p.nwx, p.shift, p.H, p.W);
        if (out_row < 0) return;                             // a padded position's output is cropped
    }
    float* orow = p.out + out_row * p.C + head * 32;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        float y[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) y[e] = Arith::value(oa, 4 * g + e) * inv;
        if constexpr (Arith::kPairRows)
            if (p.pair) { Arith::store_pair4(orow + 8 * g, h, y); continue; }
        *reinterpret_cast<float4*>(orow + 8 * g + 4 * h) = make_float4(y[0], y[1], y[2], y[3]);
    }
}

// Both row orders of the window kernel behind one set of checks.  Window order (token_order = false): p holds nwin
// windows of a win_rows x win_cols grid (p.nwy, p.nwx), rows win * 49 + position.  Token order: p holds the B maps'
// H x W tokens and the qkv bias; the window grid is worked out here.  `name` is the entry point, for the messages.
template <class Arith>
static int tok_window_attention_launch(const char* name, bool token_order, int B, TokAttnParams p, void* stream)
{
    if (token_order) {
        AL3D_REQUIRE(B >= 0 && p.H >= 1 && p.W >= 1 && (int64_t)B * p.H * p.W < ((int64_t)1 << 31), "%s: bad map size", name);
        if (B == 0) return AL3D_OK;
        AL3D_REQUIRE(p.qkv && p.bias && p.table && p.out, "%s: null pointer (a model without qkv bias passes zeros)", name);
        p.nwy = (p.H + TK_WS - 1) / TK_WS;
        p.nwx = (p.W + TK_WS - 1) / TK_WS;
        p.nwin = B * p.nwy * p.nwx;
    } else {
        AL3D_REQUIRE(p.qkv && p.table && p.out, "%s: null pointer", name);
    }
    AL3D_REQUIRE(p.nwin >= 0 && p.heads >= 1 && p.C == p.heads * 32, "%s: C=%d must be heads (%d) x 32", name, p.C, p.heads);
    AL3D_REQUIRE(token_order || (p.nwy >= 1 && p.nwx >= 1 && p.nwin % (p.nwy * p.nwx) == 0),
                 "%s: nwin=%d is not a whole number of %d x %d window grids", name, p.nwin, p.nwy, p.nwx);
    AL3D_REQUIRE(p.shift >= 0 && p.shift < TK_WS, "%s: shift=%d outside [0, 7)", name, p.shift);
    AL3D_REQUIRE((((uintptr_t)p.qkv | (uintptr_t)p.out | (uintptr_t)p.bias) & 15) == 0,
                 token_order ? "%s: qkv / bias / out must be 16-byte aligned" : "%s: qkv / out must be 16-byte aligned", name);
    if (p.nwin == 0) return AL3D_OK;
    const int64_t items = (int64_t)p.nwin * p.heads;
    AL3D_REQUIRE(items < ((int64_t)1 << 31), "%s: too many (window, head) items", name);
    hipLaunchKernelGGL(tok_window_attention_kernel<Arith>, dim3((unsigned)items), dim3(128), 0, (hipStream_t)stream, p);
    AL3D_CHECK_LAUNCH("tok_window_attention_kernel");
    return AL3D_OK;
}

// ------------------------------------------------------------------ multi-head attention, head dim 16, any key count
// The TransFusion query decoder (bevfusion/mmdet3d/models/utils/transformer.py:71-112: nn.MultiheadAttention with 8
// heads of 16 channels; 200 queries against themselves, then against the 180 x 180 = 32,400 BEV cells).
// One wave per (sample, head, 32-query tile, key chunk): S^T = K (Q scale)^T per 32-key tile -- head dim 16 is exactly
// one k-step of v_mfma_f32_32x32x16 -- an online softmax down the accumulator registers (running max / sum per query
// = per lane), and O^T += V^T P^T with P taken from the accumulators as the B operand (rows of O^T = the 16 channels;
// the upper half of the 32-row tile is idle).  Both operands split as in the window kernel.  Each wave writes
// (max, sum, O[16]) of its chunk; tok_mha16_combine_kernel merges the chunks.
template <class Arith>
__global__ __launch_bounds__(64) void tok_mha16_kernel(TokMhaParams p)
{
    const int lane = threadIdx.x, c = lane & 31, h = lane >> 5;
    int id = blockIdx.x;
    const int chunk = id % p.chunks; id /= p.chunks;
    const int qt = id % p.qtiles; id /= p.qtiles;
    const int head = id % p.heads;
    const int b = id / p.heads;
    const int query = qt * 32 + c;
    typename Arith::Frag q;
    {
        float qv[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (query < p.Pq) {
            const float* qp = p.q + ((int64_t)b * p.Pq + query) * p.ldq + head * 16 + 8 * h;
            const float4 a = *reinterpret_cast<const float4*>(qp), b4 = *reinterpret_cast<const float4*>(qp + 4);
            qv[0] = a.x * p.scale; qv[1] = a.y * p.scale; qv[2] = a.z * p.scale; qv[3] = a.w * p.scale;
            qv[4] = b4.x * p.scale; qv[5] = b4.y * p.scale; qv[6] = b4.z * p.scale; qv[7] = b4.w * p.scale;
        }
        Arith::split8(qv, q);
    }
    const int key0 = chunk * p.keys_per_chunk;
    const int key1 = key0 + p.keys_per_chunk < p.Pk ? key0 + p.keys_per_chunk : p.Pk;
    const float* kb = p.k + (int64_t)b * p.Pk * p.ldk + head * 16;
    const float* vb = p.v + (int64_t)b * p.Pk * p.ldv + head * 16;
    float run_max = -INFINITY, run_sum = 0.f;
    typename Arith::Acc oa = {};
    for (int kt = key0; kt < key1; kt += 32) {
        // K tile: A operand, lane (key c, half h) holds K[key][8 h .. 8 h + 7]
        typename Arith::Frag k;
        {
            float kv[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            if (kt + c < key1) {
                const float* kp = kb + (int64_t)(kt + c) * p.ldk + 8 * h;
                const float4 a = *reinterpret_cast<const float4*>(kp), b4 = *reinterpret_cast<const float4*>(kp + 4);
                kv[0] = a.x; kv[1] = a.y; kv[2] = a.z; kv[3] = a.w; kv[4] = b4.x; kv[5] = b4.y; kv[6] = b4.z; kv[7] = b4.w;
            }
            Arith::split8(kv, k);
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
        typename Arith::Acc sa = {};
        Arith::mac(k, q, sa);
        f32x16 sm;
        float mx = run_max;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int key = kt + (r & 3) + 8 * (r >> 2) + 4 * h;
            const float v = key < key1 ? Arith::value(sa, r) : -INFINITY;
            sm[r] = v;
            mx = fmaxf(mx, v);
        }
        mx = fmaxf(mx, __shfl_xor(mx, 32));              // every tile holds at least one real key: mx is finite
        const float resc = __builtin_amdgcn_exp2f((run_max - mx) * 1.44269504088896340736f);     // 0 on the first tile
        float sum = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float e = tk_exp(sm[r] - mx);
            sm[r] = e;
            sum += e;
        }
        sum += __shfl_xor(sum, 32);
        run_sum = run_sum * resc + sum;
        run_max = mx;
        Arith::rescale(oa, resc);
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            float pv[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) pv[e] = sm[8 * s + e];
            typename Arith::Frag v, pr;
            Arith::split8(vv[s], v);
            Arith::split8(pv, pr);
            Arith::mac(v, pr, oa);
        }
    }
    // rows of O^T: d = (r & 3) + 8 (r >> 2) + 4 h; d < 16 <=> r < 8
    float* o = p.part + ((((int64_t)b * p.heads + head) * p.chunks + chunk) * (p.qtiles * 32) + query) * 18;
    if (h == 0) { o[0] = run_max; o[1] = run_sum; }
#pragma unroll
    for (int r = 0; r < 8; ++r) o[2 + (r & 3) + 8 * (r >> 2) + 4 * h] = Arith::value(oa, r);
}

// the work split of tok_mha16_kernel: 32-query tiles, and the keys in equal chunks of at most 1,024 (a multiple of 32)
// with no empty chunk -- every partial holds at least one key
static inline void tok_mha16_plan(int Pq, int Pk, int& qtiles, int& chunks, int& keys_per_chunk)
{
    qtiles = (Pq + 31) / 32;
    keys_per_chunk = (int)al3d_align(al3d_cdiv(Pk, (Pk + 1023) / 1024), 32);
    chunks = (int)al3d_cdiv(Pk, keys_per_chunk);
}

template <class Arith>
static int tok_mha16_launch(const char* name, const float* q, int ldq, const float* k, int ldk, const float* v, int ldv,
                            int B, int heads, int Pq, int Pk, float scale, float* out, int ldo, void* workspace,
                            void* stream)
{
    AL3D_REQUIRE(q && k && v && out && workspace, "%s: null pointer", name);
    AL3D_REQUIRE(B >= 1 && heads >= 1 && Pq >= 1 && Pk >= 1, "%s: bad shape", name);
    AL3D_REQUIRE(ldq >= heads * 16 && ldk >= heads * 16 && ldv >= heads * 16 && ldo >= heads * 16 && ldq % 4 == 0 && ldk % 4 == 0,
                 "%s: row pitches must cover heads x 16 channels (q, k pitches multiples of 4)", name);
    AL3D_REQUIRE((((uintptr_t)q | (uintptr_t)k) & 15) == 0, "%s: q / k must be 16-byte aligned", name);
    TokMhaParams p;
    p.q = q; p.k = k; p.v = v; p.part = (float*)workspace;
    p.B = B; p.heads = heads; p.Pq = Pq; p.Pk = Pk; p.ldq = ldq; p.ldk = ldk; p.ldv = ldv;
    tok_mha16_plan(Pq, Pk, p.qtiles, p.chunks, p.keys_per_chunk);
    p.scale = scale;
    const int64_t waves = (int64_t)B * heads * p.qtiles * p.chunks;
    AL3D_REQUIRE(waves < ((int64_t)1 << 31), "%s: too many work items", name);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(tok_mha16_kernel<Arith>, dim3((unsigned)waves), dim3(64), 0, s, p);
    AL3D_CHECK_LAUNCH("tok_mha16_kernel");
    const int64_t n = (int64_t)B * heads * Pq * 16;
    hipLaunchKernelGGL(tok_mha16_combine_kernel, dim3((unsigned)al3d_cdiv(n, 256)), dim3(256), 0, s, (const float*)workspace, B,
                       heads, p.chunks, p.qtiles * 32, Pq, out, ldo);
    AL3D_CHECK_LAUNCH("tok_mha16_combine_kernel");
    return AL3D_OK;
}
