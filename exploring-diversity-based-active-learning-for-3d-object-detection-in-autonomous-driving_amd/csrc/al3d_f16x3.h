// The f16x3 arithmetic: fp32-class products with THREE f16 matrix-core products per MAC (gfx950).  Device-only; the one
// definition behind conv2d_f16x3.hip, conv2d_res.hip, conv2d_wino.hip, tokens.hip (+ tok_attention.h), the f16x3 sparse
// kernels (glds_common.h, spconv_wave.hip, spconv_glds.hip, spconv_rng.hip, spconv_blk.hip, spconv_l0.hip) and sp_rows.h.
//
// f16 carries 11 significand bits, so two pieces hold 22-23 of an fp32 value's 24 (bf16 needs
// three pieces and six products for the same, al3d_bf16x6.h).  What f16 lacks is exponent
// range; the split is arranged to spend as little of it as possible:
//
//   activation x (any |x| < 65504):  xh = f16(x)                A0
//                                    xl = f16((x - xh) * 2^11)  A1   (residual lifted by 2^11)
//   weight w, pre-scaled once per layer by a power of two so that max|ws| <= 2^14:
//                                    wh = f16(ws)               B0
//                                    wl = f16(ws - wh)          B1
//                                    wd = wh * 2^-11            B2   (derived in registers from the B0
//                                         fragment with v_pk_mul_f16; exact: wh >= 2^-3 for every
//                                         weight above 2^-17 max|w|, f16 subnormal rounding below)
//   x*ws = A0*B0 + A0*B1 + A1*B2 + (dropped xl*wl term <= 2^-24 |x ws|)
//
// All three products go into ONE fp32 accumulator (v_mfma_f32_32x32x16_f16, products exact), smallest first
// (f3_mac3); the weight scale 2^-s is folded into the per-channel BN scale on the host (exact).
// Per-product relative error <= ~3 * 2^-24, i.e. the size of one fp32 rounding, for |x| >= 2^-14.
// Below that xh is an f16 subnormal (v_cvt_f16_f32 and the gfx950 matrix core both keep them --
// measured, tools/probe_f16x3.py) with absolute error 2^-25, of which the lifted residual recovers
// eleven more bits: absolute representation error <= 2^-36 everywhere.  Measured against fp64
// (max error as a fraction of sum|a*b|, lognormal activations of typical magnitude m):
//      m = 1 .. 1e-5: 2.6e-7 .. 3.2e-7  (fp32-input MFMA kernel: 4.2e-7 .. 5.3e-7, bf16x6: 3.1e-7 .. 4.4e-7)
//      m = 1e-6: 1.4e-6 (and short K=32 sums already at m = 1e-5) -- the envelope: tensors whose
// typical magnitude is within [1e-4, 6e4].
// An activation >= 65504 turns into inf/NaN in the output, never a plausible number -- the sweep
// checks its embeddings for finiteness and names AL3D_MATH=bf16x6 (full fp32 range) as the way out.
//
// Whoever changes the split, the lift or the product order changes it here, for every kernel at once.
#pragma once
#include "conv2d_tile.h"      // f32x16, mfma32_crow

typedef float f32x4 __attribute__((ext_vector_type(4)));        // native vector: inline-asm register operands
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) void lds_void;         // operands of __builtin_amdgcn_global_load_lds
typedef const __attribute__((address_space(1))) void gbl_void;

constexpr float F3_LIFT = 2048.0f;                // 2^11: the residual's lift
constexpr float F3_UNLIFT = 0.00048828125f;       // 2^-11: wd = wh * 2^-11; value = main + 2^-11 * correction

// ---- the split of one activation: h = f16(x), l = f16((x - h) * 2^11)
// Not pinned: for values the kernel LOADED (the staged loaders, the LDS-DMA fragments) -- a pin only costs them their
// packed conversions.
__device__ __forceinline__ void f3_split(float x, _Float16& h, _Float16& l)
{
    h = (_Float16)x;                                  // subnormal below 2^-14 (kept: see above)
    l = (_Float16)__builtin_fmaf((float)h, -F3_LIFT, x * F3_LIFT);   // == (x - h) * 2^11 exactly; one v_fma_mix
}
// Pinned: for a caller whose PRODUCER arithmetic the compiler can see (x = a * b computed in the same kernel: the fused
// MLP's GELU output, the attention's probabilities and normalised rows).
__device__ __forceinline__ void f3_split_pinned(float x, _Float16& h, _Float16& l)
{
    // x is pinned to ONE rounded fp32 value first: with the producer's arithmetic visible (x = a * b), the compiler may
    // otherwise feed the residual below from the unrounded product while h rounds the rounded one -- at an f16 tie the
    // two then disagree by a whole f16 ulp (seen in the fused MLP: GELU output 0.27600098, low part with the wrong sign)
    asm volatile("" : "+v"(x));
    h = (_Float16)x;
    float hf = (float)h;
    asm volatile("" : "+v"(hf));                                     // the residual is taken against THIS h
    l = (_Float16)__builtin_fmaf(hf, -F3_LIFT, x * F3_LIFT);         // (x - h) * 2^11 exactly
}
// a shared body that serves kernels of either form takes the split as a template argument (as B6SplitFn): every kernel
// keeps the form it has
typedef void (*F3SplitFn)(float, _Float16&, _Float16&);

// ---- eight values (one MFMA operand fragment) over the scalar split ...
template <F3SplitFn SPLIT = f3_split>
__device__ __forceinline__ void f3_split8(const float (&v)[8], f16x8& ph, f16x8& pl)
{
#pragma unroll
    for (int e = 0; e < 8; ++e) { _Float16 a, b; SPLIT(v[e], a, b); ph[e] = a; pl[e] = b; }
}
template <F3SplitFn SPLIT = f3_split>
__device__ __forceinline__ void f3_split8(const f32x4& lo, const f32x4& hi, f16x8& ph, f16x8& pl)
{
    const float v[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    f3_split8<SPLIT>(v, ph, pl);
}
template <F3SplitFn SPLIT = f3_split>
__device__ __forceinline__ void f3_split8(const float4& lo, const float4& hi, f16x8& ph, f16x8& pl)
{
    const float v[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    f3_split8<SPLIT>(v, ph, pl);
}
__device__ __forceinline__ void f3_split4(const float4& v, f16x4& h, f16x4& l)
{
    const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) { _Float16 a, b; f3_split(e[i], a, b); h[i] = a; l[i] = b; }
}

// ---- ... and pair-wise, with packed conversions (3 instructions per element instead of 5; the same bits): the "pair
// row" form, 8 floats -> (xh[8], xl'[8]) as two 16-byte words
__device__ __forceinline__ void sp_split8(const float (&v)[8], uint4& hi, uint4& lo)
{
    unsigned h[4], l[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const f32x2 x = {v[2 * e], v[2 * e + 1]};
        const f16x2 xh = __builtin_convertvector(x, f16x2);
        // (x - xh) * 2^11 == fma(xh, -2^11, x * 2^11) exactly (power-of-two scalings, exact residual)
        const f32x2 r = {__builtin_fmaf((float)xh[0], -F3_LIFT, x[0] * F3_LIFT),
                         __builtin_fmaf((float)xh[1], -F3_LIFT, x[1] * F3_LIFT)};
        h[e] = __builtin_bit_cast(unsigned, xh);
        l[e] = __builtin_bit_cast(unsigned, __builtin_convertvector(r, f16x2));
    }
    hi = make_uint4(h[0], h[1], h[2], h[3]);
    lo = make_uint4(l[0], l[1], l[2], l[3]);
}
// (xh[8], xl'[8]) -> xh + xl' * 2^-11
__device__ __forceinline__ void sp_unsplit8(const uint4& hi, const uint4& lo, float (&v)[8])
{
    const f16x8 h = __builtin_bit_cast(f16x8, hi), l = __builtin_bit_cast(f16x8, lo);
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = __builtin_fmaf((float)l[e], F3_UNLIFT, (float)h[e]);
}
// the pair-wise split on the operand types in use, results as MFMA fragments
__device__ __forceinline__ void f3_split8p(const float (&v)[8], f16x8& ph, f16x8& pl)
{
    uint4 h, l;
    sp_split8(v, h, l);
    ph = __builtin_bit_cast(f16x8, h);
    pl = __builtin_bit_cast(f16x8, l);
}
__device__ __forceinline__ void f3_split8p(const f32x4& lo, const f32x4& hi, f16x8& ph, f16x8& pl)
{
    const float v[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    uint4 h, l;
    sp_split8(v, h, l);
    ph = __builtin_bit_cast(f16x8, h);
    pl = __builtin_bit_cast(f16x8, l);
}
__device__ __forceinline__ void f3_split8p(const float4& lo, const float4& hi, f16x8& ph, f16x8& pl)
{
    const float v[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    uint4 h, l;
    sp_split8(v, h, l);
    ph = __builtin_bit_cast(f16x8, h);
    pl = __builtin_bit_cast(f16x8, l);
}
// pair-wise, inputs pinned first (see f3_split_pinned: the high part and the residual must see the same rounded value)
__device__ __forceinline__ void f3_split8p_pinned(float (&v)[8], f16x8& ph, f16x8& pl)
{
#pragma unroll
    for (int e = 0; e < 8; ++e) asm volatile("" : "+v"(v[e]));
    f3_split8p(v, ph, pl);
}

// ---- weights: wd fragment = wh fragment * 2^-11 (packed f16 multiplies; the compiler emits v_pk_mul_f16)
__device__ __forceinline__ f16x8 f3_lift_down(const f16x8& wh)
{
    return wh * (_Float16)F3_UNLIFT;
}
__device__ __forceinline__ uint4 f3_lift_down(const uint4& wh)
{
    return __builtin_bit_cast(uint4, f3_lift_down(__builtin_bit_cast(f16x8, wh)));
}

// ---- products (fragments by value: by reference hipcc allocates the callers' split registers differently, see
// profiles/f16x3_header_parent_vs_tree.md)
__device__ __forceinline__ f32x16 f3_mfma32(f16x8 a, f16x8 b, f32x16 c)
{
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ f32x4 f3_mfma16(f16x8 a, f16x8 b, f32x4 c)
{
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
}
// The product triple in its ONE order, smallest first: xl' * wd, xh * wl, xh * wh (wd = f3_lift_down(wh)).  Every
// kernel gives every accumulator its products in this order, which is why all structures of a layer give the same bits;
// the asm blocks (gl_read_next_mfma in glds_common.h, f3_ring_gemm below) and the kernels that interleave several
// tiles product-major spell the same order out.  XA: the activation is the MFMA's A operand (rows of C = pixels); the
// token kernels that keep C transposed (rows = output channels) pass false.
template <bool XA = true>
__device__ __forceinline__ void f3_mac3(f16x8 ah, f16x8 al, f16x8 wh, f16x8 wl, f16x8 wd,
                                        f32x16& acc)
{
    acc = XA ? f3_mfma32(al, wd, acc) : f3_mfma32(wd, al, acc);
    acc = XA ? f3_mfma32(ah, wl, acc) : f3_mfma32(wl, ah, acc);
    acc = XA ? f3_mfma32(ah, wh, acc) : f3_mfma32(wh, ah, acc);
}
template <bool XA = true>                               // the same on v_mfma_f32_16x16x32_f16
__device__ __forceinline__ void f3_mac3(f16x8 ah, f16x8 al, f16x8 wh, f16x8 wl, f16x8 wd,
                                        f32x4& acc)
{
    acc = XA ? f3_mfma16(al, wd, acc) : f3_mfma16(wd, al, acc);
    acc = XA ? f3_mfma16(ah, wl, acc) : f3_mfma16(wl, ah, acc);
    acc = XA ? f3_mfma16(ah, wh, acc) : f3_mfma16(wh, ah, acc);
}

// C fragment of v_mfma_f32_32x32x16: lane (fr, fh) holds column fr; register r holds this row of the tile
__device__ __forceinline__ int f3_crow(int r, int fh) { return mfma32_crow(r, fh); }      // conv2d_tile.h

// counted wait for this wave's outstanding global loads / LDS-DMA requests
template <int N> __device__ __forceinline__ void f3_wait_vm()
{
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// ---- 1-D grid -> (tile, column block).  Blocks with equal blockIdx % 8 share an XCD and its L2,
// so the column blocks of one tile get ids that differ by 8: they run on the same XCD at
// about the same time and the second one finds the tile's activations in L2 instead of HBM (the
// 1x1 layers are bandwidth-bound: 42 flop per byte).  Grid = ceil(ntiles / 8) * 8 * nblocks.
// band: each XCD (blockIdx % 8) walks ONE contiguous band of tiles in raster order, the column
// blocks of a tile back to back -- so that the tiles resident on an XCD at any moment are spatial neighbours (the 3x3 kernels'
// 6 x 34 halos overlap: rows shared with the tile above / below are L2 hits instead of second HBM reads) and the second column
// block still finds its activations in L2.  Otherwise ("rr"): tiles dealt round-robin over the XCDs.
// false: a padding block of the last group (uniform).
__device__ __forceinline__ bool f3_tile_of_block(int ntiles, int nblocks, bool band, int& tile, int& nblk)
{
    if (band) {
        const int k = blockIdx.x & 7, t = blockIdx.x >> 3;
        const int j = t / nblocks;
        nblk = t - j * nblocks;
        const int q8 = ntiles >> 3, r8 = ntiles & 7;
        tile = k * q8 + (k < r8 ? k : r8) + j;
        return j < q8 + (k < r8 ? 1 : 0);
    }
    const int id = blockIdx.x, span = 8 * nblocks;
    const int grp = id / span, rem = id - grp * span;
    nblk = rem >> 3;
    tile = grp * 8 + (rem & 7);
    return tile < ntiles;
}

// ---- the LDS-DMA ring GEMM: a 128 x 128 tile, 16 channels per step, 256 threads = four waves of 64 x 64 (wave w =
// (wm, wn) = (w & 1, w >> 1)), behind conv2d_f16x3_dma2_kernel and tok_linear_f16x3_kernel (and, piece by piece,
// conv2d_f16x3_dma_kernel).
// A stage = 8 KB of A (128 rows x 16 channels: raw fp32, or pair rows) + 8 KB of B (128 output channels x 16 x {wh, wl},
// al3d_pack_f16x3_dma's image), written by four `global_load_lds_dwordx4` per wave.  A: wave w fetches rows
// 32 w .. 32 w + 31 as two 1 KB pieces, piece i = rows 2 jg + i of lanes (jg, sg) = (lane >> 2, lane & 3); the LDS side
// of a DMA is lane-linear, so bank conflicts are handled on the SOURCE side: lane (r, sg) fetches 16-byte chunk
// sg ^ f3_ring_swz(r).  B: wave w copies the 2 KB quarter w of the stage image as it is.
#define F3_RING_STAGE 16384
#define F3_RING_BOFF 8192
__device__ __forceinline__ int f3_ring_swz(int r) { return (r & 1) | (((r >> 3) & 1) << 1); }

// fragment side: lane (fr, fh) reads chunks 2 fh, 2 fh + 1 of row fr of M-tiles 2 wm, 2 wm + 1 (a0 / a1, second tile at
// +2048) and chunk fh of weight rows wn * 64 + {0, 32} + fr of both planes (b: wh, +4096: wl, +1024: the second tile)
struct F3RingOffs {
    unsigned a0, a1, b;
};
__device__ __forceinline__ F3RingOffs f3_ring_offsets(int wm, int wn, int fr, int fh)
{
    F3RingOffs o;
    o.a0 = (unsigned)(wm * 4096 + (fr & 1) * 1024 + (fr >> 1) * 64 + (((2 * fh) ^ f3_ring_swz(fr)) * 16));
    o.a1 = (unsigned)(wm * 4096 + (fr & 1) * 1024 + (fr >> 1) * 64 + (((2 * fh + 1) ^ f3_ring_swz(fr)) * 16));
    o.b = (unsigned)(F3_RING_BOFF + (wn * 64 + fr) * 32 + ((fh ^ ((fr >> 3) & 1)) * 16));
    return o;
}
// the MFMA operands of one step
struct F3RingOps {
    f16x8 ah[2], al[2], wh[2], wl[2], wd[2];
};
// A stage's fragments: the two A tiles raw (r0, r1: low / high 16 bytes) and the weight planes of both column tiles.
// LDS reads are inline asm with their own lgkmcnt wait: hipcc cannot see that a DMA writes LDS and would otherwise
// drain vmcnt(0) before every read it cannot disambiguate.  sb = byte address of the stage.
__device__ __forceinline__ void f3_ring_read(f32x4& r0l, f32x4& r0h, f32x4& r1l, f32x4& r1h, f16x8& wh0, f16x8& wl0, f16x8& wh1,
                                             f16x8& wl1, unsigned sb, const F3RingOffs& off)
{
    asm volatile("ds_read_b128 %0, %8\n\t"
                 "ds_read_b128 %1, %9\n\t"
                 "ds_read_b128 %2, %8 offset:2048\n\t"
                 "ds_read_b128 %3, %9 offset:2048\n\t"
                 "ds_read_b128 %4, %10\n\t"
                 "ds_read_b128 %5, %10 offset:4096\n\t"
                 "ds_read_b128 %6, %10 offset:1024\n\t"
                 "ds_read_b128 %7, %10 offset:5120\n\t"
                 "s_waitcnt lgkmcnt(0)"
                 : "=&v"(r0l), "=&v"(r0h), "=&v"(r1l), "=&v"(r1h), "=&v"(wh0), "=&v"(wl0), "=&v"(wh1), "=&v"(wl1)
                 : "v"(sb + off.a0), "v"(sb + off.a1), "v"(sb + off.b) : "memory");
}

// c[i][j] = A B over `total` steps through a ring of NS stages at LDS byte address smem_base (NS * F3_RING_STAGE bytes,
// 1 KB aligned).  issue(stage): the kernel's own address generation -- requests the NEXT step's four DMAs into `stage`
// and advances its cursor; steps past the end must re-fetch the last one (the DMA count per step stays 4).
// The kernel fills the ring first -- issue(0) .. issue(NS - 1), in that order, nothing else outstanding -- and then
// calls this; from there on the stage / fill counters and every wait are the ring's.  (With the fill loop in here hipcc
// compiled the convolution's out-of-image selects of the first requests as branches: +140 .. +350 instructions and,
// for the deconvolution, 7 more registers.)
// IN_PAIR: A arrives as pair rows (the 32 bytes of a fragment ARE (xh[8], xl'[8])), otherwise it is split with SPLIT.
// Software-pipelined: the fragments of step s+1 are read while the
// MFMAs of step s run, from ONE asm block that interleaves the eight ds_reads with the twelve MFMAs and ends in
// the lgkmcnt wait -- hipcc never sees a register that is still in flight.  Two operand sets alternate (the loop
// is unrolled by two), so the split of step s+1 writes registers no queued MFMA reads.  All NS stage buffers are
// in flight: a stage's buffer is refilled as soon as every wave holds its fragments in registers.
// The four accumulator chains are interleaved inside the block (dependent MFMAs are four instructions apart);
// each accumulator still receives xl'*wd, xh*wl, xh*wh in that order per step: the order of f3_mac3, the same bits.
template <int NS, bool IN_PAIR, F3SplitFn SPLIT, class Issue>
__device__ __forceinline__ void f3_ring_gemm(unsigned smem_base, int total, int wm, int wn, int lane, Issue& issue, f32x16& c00,
                                             f32x16& c01, f32x16& c10, f32x16& c11)
{
#pragma unroll
    for (int r = 0; r < 16; ++r) { c00[r] = 0.f; c01[r] = 0.f; c10[r] = 0.f; c11[r] = 0.f; }
    const F3RingOffs off = f3_ring_offsets(wm, wn, lane & 31, lane >> 5);

    F3RingOps A, B;
    auto finish = [&](F3RingOps& o, const f32x4& r0l, const f32x4& r0h, const f32x4& r1l, const f32x4& r1h) {
        if constexpr (IN_PAIR) {
            o.ah[0] = __builtin_bit_cast(f16x8, r0l); o.al[0] = __builtin_bit_cast(f16x8, r0h);
            o.ah[1] = __builtin_bit_cast(f16x8, r1l); o.al[1] = __builtin_bit_cast(f16x8, r1h);
        } else {
            f3_split8<SPLIT>(r0l, r0h, o.ah[0], o.al[0]);
            f3_split8<SPLIT>(r1l, r1h, o.ah[1], o.al[1]);
        }
        o.wd[0] = f3_lift_down(o.wh[0]);
        o.wd[1] = f3_lift_down(o.wh[1]);
    };

    {
        f3_wait_vm<4 * (NS - 1)>();                    // stage 0
        __builtin_amdgcn_s_barrier();
        f32x4 r0l, r0h, r1l, r1h;
        f3_ring_read(r0l, r0h, r1l, r1h, A.wh[0], A.wl[0], A.wh[1], A.wl[1], smem_base, off);
        finish(A, r0l, r0h, r1l, r1h);
    }
    int nstage = 1 % NS, fill = 0;
    // one step: MFMAs on `cur`, fragments of the next stage -> `nxt`
    auto step = [&](F3RingOps& cur, F3RingOps& nxt) {
        f3_wait_vm<4 * (NS - 2)>();                    // this wave's share of the next stage has landed ...
        __builtin_amdgcn_s_barrier();                  // ... everyone's has; every wave holds the current stage in registers
        issue(fill);                                   // -> the current stage's buffer
        const unsigned sb = smem_base + nstage * F3_RING_STAGE;
        f32x4 r0l, r0h, r1l, r1h;
        asm volatile("s_nop 1\n\t"
                     "ds_read_b128 %0, %22\n\t"
                     "ds_read_b128 %1, %23\n\t"
                     "v_mfma_f32_32x32x16_f16 %8, %12, %16, %8\n\t"
                     "v_mfma_f32_32x32x16_f16 %9, %12, %19, %9\n\t"
                     "ds_read_b128 %2, %22 offset:2048\n\t"
                     "ds_read_b128 %3, %23 offset:2048\n\t"
                     "v_mfma_f32_32x32x16_f16 %10, %14, %16, %10\n\t"
                     "v_mfma_f32_32x32x16_f16 %11, %14, %19, %11\n\t"
                     "ds_read_b128 %4, %24\n\t"
                     "ds_read_b128 %5, %24 offset:4096\n\t"
                     "v_mfma_f32_32x32x16_f16 %8, %13, %17, %8\n\t"
                     "v_mfma_f32_32x32x16_f16 %9, %13, %20, %9\n\t"
                     "ds_read_b128 %6, %24 offset:1024\n\t"
                     "ds_read_b128 %7, %24 offset:5120\n\t"
                     "v_mfma_f32_32x32x16_f16 %10, %15, %17, %10\n\t"
                     "v_mfma_f32_32x32x16_f16 %11, %15, %20, %11\n\t"
                     "v_mfma_f32_32x32x16_f16 %8, %13, %18, %8\n\t"
                     "v_mfma_f32_32x32x16_f16 %9, %13, %21, %9\n\t"
                     "v_mfma_f32_32x32x16_f16 %10, %15, %18, %10\n\t"
                     "v_mfma_f32_32x32x16_f16 %11, %15, %21, %11\n\t"
                     "s_waitcnt lgkmcnt(0)"
                     : "=&v"(r0l), "=&v"(r0h), "=&v"(r1l), "=&v"(r1h), "=&v"(nxt.wh[0]), "=&v"(nxt.wl[0]), "=&v"(nxt.wh[1]),
                       "=&v"(nxt.wl[1]), "+v"(c00), "+v"(c01), "+v"(c10), "+v"(c11)
                     : "v"(cur.al[0]), "v"(cur.ah[0]), "v"(cur.al[1]), "v"(cur.ah[1]),                    // 12..15
                       "v"(cur.wd[0]), "v"(cur.wl[0]), "v"(cur.wh[0]), "v"(cur.wd[1]), "v"(cur.wl[1]), "v"(cur.wh[1]),   // 16..21
                       "v"(sb + off.a0), "v"(sb + off.a1), "v"(sb + off.b)                                // 22..24
                     : "memory");
        finish(nxt, r0l, r0h, r1l, r1h);
        nstage = nstage + 1 == NS ? 0 : nstage + 1;
        fill = fill + 1 == NS ? 0 : fill + 1;
    };
    for (int s = 0; s < total; s += 2) {
        step(A, B);
        if (s + 1 < total) step(B, A);
    }
    f3_wait_vm<0>();                                   // the tail's dummy requests must not outlive the workgroup's LDS
    asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");  // the last MFMAs' results before the VALU reads them
}
