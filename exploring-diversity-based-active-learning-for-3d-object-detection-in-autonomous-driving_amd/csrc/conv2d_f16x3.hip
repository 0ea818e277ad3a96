// Dense 2-D convolution in fp32-class arithmetic with THREE f16 matrix-core products per MAC: the f16x3 arithmetic of
// al3d_f16x3.h (split, ranges, error bounds, measured envelope, product order).
//
// Same role, layouts and tiling as conv2d_bf16x6.hip: NHWC f32 activations in HBM, split while
// they are staged; weights pre-split into [2][Cout][taps][Cin] f16.  Half the MFMAs, 4 instead
// of 6 fragment reads per step, 2/3 of the LDS.  The pixel-tile side (parameter block, tile decode, input pixel, the
// untransposed epilogues, entry-point checks) is conv2d_tile.h's.
//
// Kernels in this file (all bit-identical to one another on the same layer):
//   conv3x3_f16x3_frag_kernel     3x3/s1/p1, halo in LDS, weights streamed in fragment order   (default)
//   conv3x3_f16x3_halo_kernel     3x3/s1/p1, halo and weights through LDS                      (AL3D_DENSE=lds)
//   conv2d_f16x3_bstream_kernel   any geometry, activation tile in LDS, weights streamed       (>= 24 steps)
//   conv2d_f16x3_kernel           any geometry, both tiles through LDS                         (short launches, deconv)
#include "al3d_common.h"
#include "sp_rows.h"
#include "conv2d_tile.h"
#include <stdlib.h>
#include <type_traits>

#define F3_BM 128
#define F3_BN 128
#define F3_BK 16
#define F3_LDB 48          // bytes per LDS row: 16 f16 (32 B) + 16 B pad (conflict-free b128 reads)
#define F3_TH 8
#define F3_TW 16

// This file's A/B knobs, read from the environment once per process (the same bits under every setting)
struct F3Knobs {
    int xmap;          // AL3D_F3_MAP=band (default) | rr: see f3_tile_of_block
    int frag_direct;   // AL3D_FRAG_EPI=direct: the streamed 3x3 kernel's untransposed f32 epilogue everywhere
    int frag_shape;    // AL3D_FRAG_SHAPE=2 (default) | 1 | 0: its wave shape, see al3d_conv3x3_nhwc_f16x3_frag
    int dma_stages;    // AL3D_DMA_STAGES=3 (default: 48 KB, three workgroups per CU, measured best) | 4 | 5
    int dma_pipe;      // AL3D_DMA_PIPE=1 (default: conv2d_f16x3_dma2_kernel) | 0 (conv2d_f16x3_dma_kernel)
    int dma_direct;    // AL3D_DMA_EPI=direct: the LDS-DMA kernel's untransposed dword stores everywhere
};
static const F3Knobs& f3_knobs()
{
    static const F3Knobs knobs = [] {
        F3Knobs k;
        const char* e = getenv("AL3D_F3_MAP");
        k.xmap = !(e && e[0] == 'r');
        e = getenv("AL3D_FRAG_EPI");
        k.frag_direct = e && e[0] == 'd';
        e = getenv("AL3D_FRAG_SHAPE");
        k.frag_shape = e ? atoi(e) : 2;
        e = getenv("AL3D_DMA_STAGES");
        k.dma_stages = e ? atoi(e) : 3;
        if (k.dma_stages != 3 && k.dma_stages != 4 && k.dma_stages != 5) k.dma_stages = 3;
        e = getenv("AL3D_DMA_PIPE");
        k.dma_pipe = e ? atoi(e) != 0 : 1;
        e = getenv("AL3D_DMA_EPI");
        k.dma_direct = e && e[0] == 'd';
        return k;
    }();
    return knobs;
}

struct ConvF3Params : ConvGeom {          // scale = BN scale * 2^-s, required
    const _Float16* wgt;    // [2][Cout][taps][Cin] f16 planes (wh, wl)
    int nblocks, ntiles;    // 128-channel column blocks; pixel tiles (tiles_x * tiles_y * B)
    int64_t plane;          // elements per weight plane = Cout * taps * Cin
    float* gap;             // optional [B][gap_parts][ldc]: per-workgroup channel sums of the stored values (fused GAP)
    int gap_parts;
    int xmap = f3_knobs().xmap;    // workgroup -> (pixel tile, column block) order, see f3_tile_of_block
    int io = 0;             // row formats of in / out (sp_rows.h: bit 0 = in pair pixels, bit 1 = write pair pixels); DMA kernel only
    // conv3x3_f16x3_frag_kernel, SRC = 1: the input map is given as sparse rows.  rows [n][rows_pitch] f32 (C = Cin / 2
    // channels used), bev [B,H,W,2] i32 = row of (pixel, z) or -1 (al3d_sp_bev_index); map channel c * 2 + z = rows[row][c]
    const float* rows = nullptr;
    const int* bev = nullptr;
    int rows_pitch = 0;
};

// grid of f3_tile_of_block (al3d_f16x3.h); every kernel here passes p.xmap as its band flag
static inline unsigned f3_grid(const ConvF3Params& p)
{
    return (unsigned)(al3d_cdiv(p.ntiles, 8) * 8 * p.nblocks);
}

#define F3_IC(v) std::integral_constant<int, v>{}

template <int MODE>
__global__ __launch_bounds__(256, 2) void conv2d_f16x3_kernel(ConvF3Params p)
{
    __shared__ __attribute__((aligned(16))) unsigned char As[2][2][F3_BM * F3_LDB];   // [buf][plane]
    __shared__ __attribute__((aligned(16))) unsigned char Bs[2][2][F3_BN * F3_LDB];
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int wm = wave & 1, wn = wave >> 1;
    int tile, nblk;
    if (!f3_tile_of_block(p.ntiles, p.nblocks, p.xmap, tile, nblk)) return;     // padding block of the last group (uniform)
    int tx_, ty_, b;
    conv_tile_decode(tile, p.tiles_x, p.tiles_y, tx_, ty_, b);
    const int n0 = nblk * F3_BN;
    const int taps = MODE == 0 ? p.ksize * p.ksize : 1;
    const int tap0 = MODE == 0 ? 0 : blockIdx.z;
    const int wtaps = MODE == 0 ? taps : 4;

    const int aq = tid & 3, ar = tid >> 2;            // piece, row (0..63), +64 on pass 1
    int py[2], px[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int m = ar + 64 * i;
        py[i] = ty_ * F3_TH + m / F3_TW;
        px[i] = tx_ * F3_TW + m % F3_TW;
    }
    const int bq = tid & 1, br = tid >> 1;
    const int kchunks = p.Cin / F3_BK;
    const int nsteps = taps * kchunks;

    float4 ra[2];
    uint4 rb[2];
    auto load_step = [&](int step) {
        const int tap = step / kchunks, c0 = (step - tap * kchunks) * F3_BK;
        const int ky = MODE == 0 ? tap / p.ksize : 0, kx = MODE == 0 ? tap % p.ksize : 0;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            int iy, ix;
            const bool ok = conv_tap_pixel<MODE>(p, py[i], px[i], ky, kx, iy, ix);
            ra[i] = conv_load4(p, ok, b, iy, ix, c0 + 4 * aq);
        }
        const int n = n0 + br;
#pragma unroll
        for (int pl = 0; pl < 2; ++pl)
            rb[pl] = n < p.Cout ? *reinterpret_cast<const uint4*>(
                                      p.wgt + pl * p.plane + ((int64_t)n * wtaps + tap0 + tap) * p.Cin + c0 + 8 * bq)
                                : make_uint4(0u, 0u, 0u, 0u);
    };
    auto store_step = [&](int buf) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            f16x4 h, l;
            f3_split4(ra[i], h, l);
            const int off = (ar + 64 * i) * F3_LDB + 8 * aq;
            *reinterpret_cast<f16x4*>(&As[buf][0][off]) = h;
            *reinterpret_cast<f16x4*>(&As[buf][1][off]) = l;
        }
#pragma unroll
        for (int pl = 0; pl < 2; ++pl)
            *reinterpret_cast<uint4*>(&Bs[buf][pl][br * F3_LDB + 16 * bq]) = rb[pl];
    };

    f32x16 acc[2][2];
    conv_acc_clear(acc);

    load_step(0);
    store_step(0);
    __syncthreads();
    const int fr = lane & 31, fh = lane >> 5;
    for (int step = 0; step < nsteps; ++step) {
        const int buf = step & 1;
        if (step + 1 < nsteps) load_step(step + 1);
        f16x8 a[2][2], bb[3][2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
#pragma unroll
            for (int pl = 0; pl < 2; ++pl) {
                a[pl][t] = *reinterpret_cast<const f16x8*>(&As[buf][pl][(wm * 64 + t * 32 + fr) * F3_LDB + 16 * fh]);
                bb[pl][t] = *reinterpret_cast<const f16x8*>(&Bs[buf][pl][(wn * 64 + t * 32 + fr) * F3_LDB + 16 * fh]);
            }
            bb[2][t] = f3_lift_down(bb[0][t]);
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) f3_mac3(a[0][i], a[1][i], bb[0][j], bb[1][j], bb[2][j], acc[i][j]);
        if (step + 1 < nsteps) store_step(buf ^ 1);
        __syncthreads();
    }

    // epilogue with the fused GAP partials (conv2d_tile.h)
    conv_store_patch<MODE, F3_TH, F3_TW, 2, 2, false, true>(p, acc, b, ty_, tx_, wm, n0 + wn * 64, tap0, lane, p.gap, p.gap_parts);
}

// out[b][c] = (sum over the parts, ascending) / count
__global__ __launch_bounds__(64) void gap_parts_reduce_kernel(const float* __restrict__ gap, int parts, int C, float count,
                                                               float* __restrict__ out)
{
    gap_cols_reduce(gap, parts, C, count, out);
}

// ------------------------------------------------------------------ 3x3 / stride 1 / pad 1
// Halo-staged kernel: the 6x34-pixel input halo of a 4x32 output tile is split and staged once
// per 16-channel chunk, the nine taps read their A fragments from it at shifted rows; only the
// weight tile changes per tap.  Output tile = 4 rows x 32 columns: lane r of an M-tile is column
// r, so the 32 lanes of a fragment read 32 consecutive halo rows (conflict-free ds_read_b128 at
// a 48-byte pitch).
//
// With three MFMAs per tile pair a step holds only 12 x 32 matrix-core cycles per wave, far less
// than an L2 round trip, so -- unlike the bf16x6 kernel this grew from -- nothing may wait inside
// a step.  Global step s = chunk * 9 + tap; everything below is software-pipelined over s:
//   * weights: global load of B(s+3) is issued at the top of step s into register set (s+1)&1;
//     the set loaded one step earlier, B(s+2), is written to LDS buffer (s+2)%3 at the end of
//     step s -- two full steps between issue and use;
//   * three weight buffers (two planes each; the third operand is derived) in LDS (32-byte rows, 16-byte halves XOR-swizzled by bit 3 of the
//     row: conflict-free b128 reads and writes without padding): B(s+1) is read by the fragment
//     prefetch of step s, B(s) was read during step s-1, B(s+2) is being written;
//   * fragments of step s+1 are read into the second register set while the MFMAs of step s run;
//   * the halo is double-buffered by chunk parity: loads for chunk c+1 are issued at taps 0 and 3
//     of chunk c (two halves, to halve the staging registers), split and stored at taps 2 and 5,
//     published by those taps' barriers, first read at tap 8;
//   * one barrier per step; 9 is odd, so two chunks are unrolled to keep every register-set
//     and buffer index a compile-time constant;
//   * every global load is unconditional (out-of-image pixels, rows beyond Cout and the steps
//     past the end read a zero word / a clamped address): a branch around a VMEM op would make
//     hipcc wait for vmcnt(0) at the next use and serialise the pipeline.
#define G3_TH 4
#define G3_TW 32
#define G3_HH (G3_TH + 2)
#define G3_HW (G3_TW + 2)
#define G3_HP (G3_HH * G3_HW)          // 204 halo pixels
#define G3_BROW 32                     // bytes per weight row in LDS (16 f16, swizzled halves)

__device__ uint4 g_f3_zero16;          // 16 zero bytes (device globals are zero-initialised)

__global__ __launch_bounds__(256, 2) void conv3x3_f16x3_halo_kernel(ConvF3Params p)
{
    __shared__ __attribute__((aligned(16))) unsigned char Ah[2][2][G3_HP * F3_LDB];      // [chunk parity][plane] 39.2 KB
    __shared__ __attribute__((aligned(16))) unsigned char Bs[3][2][F3_BN * G3_BROW];     // [step % 3][plane]     24.6 KB
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int wm = wave & 1, wn = wave >> 1;
    const int fr = lane & 31, fh = lane >> 5;
    int tile, nblk;
    if (!f3_tile_of_block(p.ntiles, p.nblocks, p.xmap, tile, nblk)) return;     // padding block of the last group (uniform)
    int tx_, ty_, b;
    conv_tile_decode(tile, p.tiles_x, p.tiles_y, tx_, ty_, b);
    const int n0 = nblk * F3_BN;
    const int y0 = ty_ * G3_TH - 1, x0 = tx_ * G3_TW - 1;       // image coords of halo (0,0)
    const int nchunks = p.Cin / F3_BK;
    const int bq = tid & 1, br = tid >> 1;
    const float* zero = reinterpret_cast<const float*>(&g_f3_zero16);

    // ---- halo: 204 pixels x 4 float4 pieces = 816 pieces over 4 passes of 256 threads
    float4 rh[2];                                    // the halo travels in two halves (8 VGPRs, not 16)
    auto load_halo = [&](int chunk, int half) {
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int i = 2 * half + k;
            const int piece = tid + 256 * i;
            const int hp = piece >> 2, q = piece & 3;
            int iy, ix;
            const bool ok = conv_halo_pixel<G3_HW>(p, y0, x0, hp, hp < G3_HP, iy, ix);
            rh[k] = conv_load4(p, ok, b, iy, ix, chunk * F3_BK + 4 * q, zero);
        }
    };
    auto store_halo = [&](int buf, int half) {
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int piece = tid + 256 * (2 * half + k);
            const int hp = piece >> 2, q = piece & 3;
            if (hp >= G3_HP) continue;
            f16x4 h, l;
            f3_split4(rh[k], h, l);
            const int off = hp * F3_LDB + 8 * q;
            *reinterpret_cast<f16x4*>(&Ah[buf][0][off]) = h;
            *reinterpret_cast<f16x4*>(&Ah[buf][1][off]) = l;
        }
    };
    // ---- weights: this thread's 16-byte piece of row n0+br, three planes
    const int nb = n0 + br;
    const bool nb_ok = nb < p.Cout;
    const _Float16* wrow = nb_ok ? p.wgt + (int64_t)nb * 9 * p.Cin + 8 * bq
                                 : reinterpret_cast<const _Float16*>(zero);
    const int64_t wplane = nb_ok ? p.plane : 0;
    const int wtap = nb_ok ? p.Cin : 0, wchunk = nb_ok ? F3_BK : 0;
    uint4 rb0[2], rb1[2];                            // two register sets (named: an [2][2] array went to scratch)
    auto load_b = [&](auto set_, int chunk, int tap) {
#pragma unroll
        for (int pl = 0; pl < 2; ++pl) {
            const uint4 v = *reinterpret_cast<const uint4*>(wrow + pl * wplane + tap * wtap + chunk * wchunk);
            if constexpr (decltype(set_)::value == 0) rb0[pl] = v; else rb1[pl] = v;
        }
    };
    const int bw_off = br * G3_BROW + 16 * (bq ^ ((br >> 3) & 1));
    auto store_b = [&](auto set_, int buf) {
#pragma unroll
        for (int pl = 0; pl < 2; ++pl) {
            if constexpr (decltype(set_)::value == 0) *reinterpret_cast<uint4*>(&Bs[buf][pl][bw_off]) = rb0[pl];
            else *reinterpret_cast<uint4*>(&Bs[buf][pl][bw_off]) = rb1[pl];
        }
    };

    f32x16 acc[2][2];
    conv_acc_clear(acc);

    const int a_off = ((2 * wm) * G3_HW + fr) * F3_LDB + 16 * fh;
    const int b_off = (wn * 64 + fr) * G3_BROW + 16 * (fh ^ ((fr >> 3) & 1));   // +32 rows keeps bit 3
    f16x8 fa[2][2][2], fb[2][2][2];                   // [set][plane][tile]
    // fragment reads are issued plane by plane, each right after the MFMA group that last used the
    // registers of the same plane in the current set (keeps ~1.5 fragment sets live, not 2)
    auto read_a = [&](int set, int pl, int hbuf, int tap) {
        const int ky = tap / 3, kx = tap % 3;
#pragma unroll
        for (int t = 0; t < 2; ++t)
            fa[set][pl][t] = *reinterpret_cast<const f16x8*>(
                &Ah[hbuf][pl][a_off + ((t + ky) * G3_HW + kx) * F3_LDB]);
    };
    auto read_b = [&](int set, int pl, int bbuf) {
#pragma unroll
        for (int t = 0; t < 2; ++t)
            fb[set][pl][t] = *reinterpret_cast<const f16x8*>(&Bs[bbuf][pl][b_off + t * 32 * G3_BROW]);
    };
    auto read_frags = [&](int set, int hbuf, int tap, int bbuf) {
        read_a(set, 1, hbuf, tap); read_b(set, 0, bbuf);
        read_b(set, 1, bbuf);
        read_a(set, 0, hbuf, tap);
    };
    auto mfma_group = [&](int set, int pa, int pb) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
                acc[i][j] = f3_mfma32(fa[set][pa][i], fb[set][pb][j], acc[i][j]);
    };
    // (product-major over the four tiles, interleaved with the step's loads and stores: f3_mac3's order, spelled out)
    auto mfma_lifted = [&](int set) {                 // xl' * (wh * 2^-11)
        f16x8 wd[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) wd[j] = f3_lift_down(fb[set][0][j]);
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
                acc[i][j] = f3_mfma32(fa[set][1][i], wd[j], acc[i][j]);
    };

    // ---- prologue: halo(0), B(0), B(1) in LDS; B(2) in flight in register set 0
    const int last = nchunks - 1;
    load_halo(0, 0);
    load_b(F3_IC(0), 0, 0);
    store_halo(0, 0);
    load_halo(0, 1);
    store_halo(0, 1);
    store_b(F3_IC(0), 0);
    load_b(F3_IC(0), 0, 1);
    store_b(F3_IC(0), 1);
    load_b(F3_IC(0), 0, 2);
    __syncthreads();
    read_frags(0, 0, 0, 0);

    // cp (chunk parity) and tap are template-level constants so that every register-set and LDS
    // buffer index is constant from the start (a loop variable, even fully unrolled, left the
    // staging arrays in scratch memory).
    auto step = [&](auto cp_, auto tap_, int chunk, int cn) {
        constexpr int cp = decltype(cp_)::value, tap = decltype(tap_)::value;
        constexpr int q = (cp + tap) & 1;             // register-set parity of this step
        // B(s+3) -> the other register set (in flight for two steps)
        if (tap < 6) load_b(F3_IC(q ^ 1), chunk, tap + 3);
        else load_b(F3_IC(q ^ 1), cn, tap - 6);
        if (tap == 0) load_halo(cn, 0);               // next chunk's halo, first half: stored at tap 2
        if (tap == 3) load_halo(cn, 1);               // second half: stored at tap 5, first read at tap 8
        __builtin_amdgcn_sched_barrier(0);            // keep the loads at the top of the step (hipcc sinks them to the stores)
        // MFMAs of step s (smallest products first: xl*wd, xh*wl, xh*wh), interleaved with the
        // fragment reads of step s+1 (halo of the next chunk after tap 8)
        constexpr int nh = tap < 8 ? cp : cp ^ 1, nt = tap < 8 ? tap + 1 : 0, nbuf = (tap + 1) % 3;
        mfma_lifted(q);
        read_a(q ^ 1, 1, nh, nt);
        mfma_group(q, 0, 1);
        read_b(q ^ 1, 1, nbuf);
        mfma_group(q, 0, 0);
        read_a(q ^ 1, 0, nh, nt); read_b(q ^ 1, 0, nbuf);
        store_b(F3_IC(q), (tap + 2) % 3);             // B(s+2), loaded during step s-1
        if (tap == 2) store_halo(cp ^ 1, 0);
        if (tap == 5) store_halo(cp ^ 1, 1);
        __syncthreads();
    };
    auto chunk_body = [&](auto cp_, int chunk) {
        const int cn = chunk < last ? chunk + 1 : chunk;         // clamped: the last chunk re-reads itself
        step(cp_, F3_IC(0), chunk, cn); step(cp_, F3_IC(1), chunk, cn); step(cp_, F3_IC(2), chunk, cn);
        step(cp_, F3_IC(3), chunk, cn); step(cp_, F3_IC(4), chunk, cn); step(cp_, F3_IC(5), chunk, cn);
        step(cp_, F3_IC(6), chunk, cn); step(cp_, F3_IC(7), chunk, cn); step(cp_, F3_IC(8), chunk, cn);
    };
    for (int chunk0 = 0; chunk0 < nchunks; chunk0 += 2) {       // nchunks is even (checked by the launcher)
        chunk_body(F3_IC(0), chunk0);
        chunk_body(F3_IC(1), chunk0 + 1);
    }

    conv_store_rows<G3_TH, G3_TW, 2, 2, false>(p, acc, b, ty_, tx_, 2 * wm, n0 + wn * 64, lane);
}

// ------------------------------------------------------------------ 3x3 / stride 1 / pad 1, weights from L2
// The kernel above is bound by LDS bandwidth, not by the matrix cores: per step a CU moves 64 KB
// of fragment reads + 16 KB of weight writes through LDS for 24 x 4 MFMAs (ablation on MI355X,
// B=32 128x128x128->128: full 537 us; without the weight staging 440; without any staging 398;
// without the barrier 536).  Here the weights never touch LDS: they are pre-arranged in HBM in
// FRAGMENT order -- [plane][Cout/32][chunk][tap][lane][8] f16, i.e. the 1 KiB a wave needs for one
// B operand is contiguous and lane-ordered -- and every wave loads its own B fragments straight
// into registers with one coalesced global_load_dwordx4 per fragment, two steps ahead (register
// ring of three sets; the steps of a wave walk its weight stream linearly).  What is left in LDS
// is the double-buffered activation halo, so a block needs only TWO barriers per chunk of nine
// taps (one before the next halo's first store -- its buffer was last read at tap 7 of the
// previous chunk -- and one after its last store), and the four waves drift freely in between.
// LDS traffic per step and CU: 83 KB -> 35 KB; L2 -> CU traffic doubles (both M-waves of a block
// load the same weights: 32 KB per step and CU, ~40 % of the vector L1's 64 B/clk).
// SHAPE 1 (round 5): a wave owns all FOUR image rows of the tile x ONE 32-channel tile instead of two rows x two tiles, so
// every weight fragment is loaded by exactly one wave of the workgroup (half the L2 -> CU weight traffic: 11.5 instead of
// 23 TB/s chip-wide on the 256 -> 256 layers) at twice the LDS fragment reads; same MFMA sequence per accumulator.
// SRC 1 (SHAPE 2 only): the input map is the sparse encoder's last level, read from its rows through a BEV row index
// (p.rows, p.bev) instead of from a dense map that is 3/4 zeros.  A 16-byte halo piece {r0[c], r1[c], r0[c+1], r1[c+1]} is
// two 8-byte loads from the pixel's two rows (z = 0, 1), a missing row reads the zero block; the LDS image is the one the
// dense map gives.  The workgroup also knows which of its six halo rows are entirely empty and skips the MFMAs whose A
// operand is such a row: they would add products of +0 to the accumulator, which leaves every accumulator (+0 at the
// start, or already non-zero) bit for bit as it was.
template <int IO = 0, int SHAPE = 0, int SRC = 0>
__global__ __launch_bounds__(256, 2) void conv3x3_f16x3_frag_kernel(ConvF3Params p)
{
    static_assert(SRC == 0 || SHAPE == 2, "the rows input is built for wave shape 2 only");
    constexpr int NI = SHAPE ? 4 : 2, NJ = SHAPE ? 1 : 2;      // M tiles (image rows) x N tiles (32 channels) per wave
    constexpr bool HALO_FAR = SHAPE == 2;
    constexpr int NHB = 2;                                    // halo buffers (a third one, dropping the tap-1 barrier, measured a tie)
    static_assert(SHAPE >= 0 && SHAPE <= 2, "wave shapes 0 / 1; 2 = 1 with the far halo prefetch");
    __shared__ __attribute__((aligned(16))) unsigned char Ah[NHB][2][G3_HP * F3_LDB];    // [chunk % NHB][plane] 39.2 KB (58.8)
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int wm = SHAPE ? 0 : (wave & 1), wn = wave >> 1;
    const int row0 = SHAPE ? 0 : 2 * wm, ch0 = SHAPE ? wave * 32 : wn * 64;      // the wave's first image row / channel in the tile
    const int fr = lane & 31, fh = lane >> 5;
    int tile, nblk;
    if (!f3_tile_of_block(p.ntiles, p.nblocks, p.xmap, tile, nblk)) return;     // padding block of the last group (uniform)
    int tx_, ty_, b;
    conv_tile_decode(tile, p.tiles_x, p.tiles_y, tx_, ty_, b);
    const int n0 = nblk * F3_BN;
    const int y0 = ty_ * G3_TH - 1, x0 = tx_ * G3_TW - 1;       // image coords of halo (0,0)
    const int nchunks = p.Cin / F3_BK;
    const int total = 9 * nchunks;
    const float* zero = reinterpret_cast<const float*>(&g_f3_zero16);

    // the next chunk's halo travels in two halves; HALO_FAR (round 5): each half has its own registers and waits FOUR steps
    // between its request and its store (two before: a step apart is ~1.5k cycles of wall time at two waves per SIMD, less than
    // an HBM round trip under load, and vmcnt retires in order, so the wait also held the weight stream back)
    float4 rh[HALO_FAR ? 4 : 2];
    int2 hrow[SRC ? 4 : 1];                                   // SRC 1: the rows (z = 0, 1) of this thread's four halo pixels
    unsigned live = 0x3f;                                     // SRC 1: bit r = halo row r holds a row (wave-uniform)
    if constexpr (SRC != 0) {
        __shared__ unsigned live_s;
        if (tid == 0) live_s = 0;
        unsigned mine = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int hp = (tid + 256 * k) >> 2;
            int iy, ix;
            const bool ok = conv_halo_pixel<G3_HW>(p, y0, x0, hp, hp < G3_HP, iy, ix);
            const int* src = p.bev + (((int64_t)b * p.H + iy) * p.W + ix) * 2;
            hrow[k] = ok ? *reinterpret_cast<const int2*>(src) : make_int2(-1, -1);
            if (hrow[k].x >= 0 || hrow[k].y >= 0) mine |= 1u << (hp / G3_HW);
        }
        __syncthreads();
        if (mine) atomicOr(&live_s, mine);
        __syncthreads();
        live = __builtin_amdgcn_readfirstlane(live_s);
    }
    auto load_halo = [&](int chunk, int half) {
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int piece = tid + 256 * (2 * half + k);
            const int hp = piece >> 2, q = piece & 3;
            if constexpr (SRC != 0) {
                const int2 r = hrow[2 * half + k];
                const int c0 = chunk * (F3_BK / 2) + 2 * q;
                const float* s0 = p.rows + (int64_t)r.x * p.rows_pitch + c0;
                const float* s1 = p.rows + (int64_t)r.y * p.rows_pitch + c0;
                const float2 a0 = *reinterpret_cast<const float2*>(r.x >= 0 ? s0 : zero);
                const float2 a1 = *reinterpret_cast<const float2*>(r.y >= 0 ? s1 : zero);
                rh[(HALO_FAR ? 2 * half : 0) + k] = make_float4(a0.x, a1.x, a0.y, a1.y);
            } else {
                int iy, ix;
                const bool ok = conv_halo_pixel<G3_HW>(p, y0, x0, hp, hp < G3_HP, iy, ix);
                rh[(HALO_FAR ? 2 * half : 0) + k] = conv_load4(p, ok, b, iy, ix, chunk * F3_BK + 4 * q, zero);
            }
        }
    };
    auto store_halo = [&](int buf, int half) {
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int piece = tid + 256 * (2 * half + k);
            const int hp = piece >> 2, q = piece & 3;
            if (hp >= G3_HP) continue;
            f16x4 h, l;
            f3_split4(rh[(HALO_FAR ? 2 * half : 0) + k], h, l);
            const int off = hp * F3_LDB + 8 * q;
            *reinterpret_cast<f16x4*>(&Ah[buf][0][off]) = h;
            *reinterpret_cast<f16x4*>(&Ah[buf][1][off]) = l;
        }
    };

    // ---- this wave's weight stream: [plane][ntile][step][lane][8]; ntile = 32 output channels
    const int NT = p.Cout >> 5;
    const int nt0 = (n0 + ch0) >> 5;
    const _Float16* bsrc[2][NJ];                      // [plane][tile]
#pragma unroll
    for (int pl = 0; pl < 2; ++pl)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
            bsrc[pl][j] = p.wgt + ((int64_t)(pl * NT + nt0 + j) * total) * 512 + lane * 8;
    f16x8 fb0[2][NJ], fb1[2][NJ], fb2[2][NJ];         // ring of three register sets [plane][tile]
    auto load_b = [&](auto ring_, int sidx) {
        constexpr int ring = decltype(ring_)::value;
#pragma unroll
        for (int pl = 0; pl < 2; ++pl)
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const f16x8 v = *reinterpret_cast<const f16x8*>(bsrc[pl][j] + (int64_t)sidx * 512);
                if constexpr (ring == 0) fb0[pl][j] = v;
                else if constexpr (ring == 1) fb1[pl][j] = v;
                else fb2[pl][j] = v;
            }
    };

    f32x16 acc[NI][NJ];
    conv_acc_clear(acc);

    const int a_off = (row0 * G3_HW + fr) * F3_LDB + 16 * fh;
    f16x8 fa[2][2][NI];                               // [set][plane][tile]
    auto read_a = [&](int set, int pl, int hbuf, int tap) {
        const int ky = tap / 3, kx = tap % 3;
#pragma unroll
        for (int t = 0; t < NI; ++t)
            fa[set][pl][t] = *reinterpret_cast<const f16x8*>(
                &Ah[hbuf][pl][a_off + ((t + ky) * G3_HW + kx) * F3_LDB]);
    };
    // the three products of f3_mac3 in its order, product-major over the tiles so that the step's other work goes between them
    auto mfma_step = [&](int set, auto ky_, const f16x8 (&fb)[2][NJ], auto&& between0, auto&& between1) {
        f16x8 wd[NJ];
#pragma unroll
        for (int j = 0; j < NJ; ++j) wd[j] = f3_lift_down(fb[0][j]);
        if constexpr (SRC != 0) {
            // the same three products per accumulator in the same order; image row i at tap row ky reads halo row i + ky
            constexpr int ky = decltype(ky_)::value;
#pragma unroll
            for (int i = 0; i < NI; ++i)
                if ((live >> (row0 + i + ky)) & 1)
#pragma unroll
                    for (int j = 0; j < NJ; ++j) acc[i][j] = f3_mfma32(fa[set][1][i], wd[j], acc[i][j]);
            between0();
#pragma unroll
            for (int i = 0; i < NI; ++i)
                if ((live >> (row0 + i + ky)) & 1)
#pragma unroll
                    for (int j = 0; j < NJ; ++j) acc[i][j] = f3_mfma32(fa[set][0][i], fb[1][j], acc[i][j]);
#pragma unroll
            for (int i = 0; i < NI; ++i)
                if ((live >> (row0 + i + ky)) & 1)
#pragma unroll
                    for (int j = 0; j < NJ; ++j) acc[i][j] = f3_mfma32(fa[set][0][i], fb[0][j], acc[i][j]);
            between1();
            return;
        }
#pragma unroll
        for (int i = 0; i < NI; ++i)
#pragma unroll
            for (int j = 0; j < NJ; ++j) acc[i][j] = f3_mfma32(fa[set][1][i], wd[j], acc[i][j]);       // xl' * wd
        between0();
#pragma unroll
        for (int i = 0; i < NI; ++i)
#pragma unroll
            for (int j = 0; j < NJ; ++j) acc[i][j] = f3_mfma32(fa[set][0][i], fb[1][j], acc[i][j]);    // xh * wl
#pragma unroll
        for (int i = 0; i < NI; ++i)
#pragma unroll
            for (int j = 0; j < NJ; ++j) acc[i][j] = f3_mfma32(fa[set][0][i], fb[0][j], acc[i][j]);    // xh * wh
        between1();
    };

    // ---- prologue: halo(0) in LDS, B(0), B(1) in flight
    const int last = nchunks - 1;
    load_halo(0, 0);
    load_b(F3_IC(0), 0);
    load_b(F3_IC(1), 1);
    store_halo(0, 0);
    load_halo(0, 1);
    store_halo(0, 1);
    __syncthreads();
    read_a(0, 1, 0, 0);
    read_a(0, 0, 0, 0);

    auto step = [&](auto cp_, auto tap_, int chunk, int cn, int hb, int hbn) {
        constexpr int cp = decltype(cp_)::value, tap = decltype(tap_)::value;
        constexpr int q = (cp + tap) & 1;             // A fragment set of this step
        constexpr int ring = (cp * 9 + tap) % 3;      // B register set of this step (18 % 3 == 0)
        const int s2 = chunk * 9 + tap + 2;           // B(s+2) -> the set used at step s-1
        load_b(F3_IC((ring + 2) % 3), s2 < total ? s2 : total - 1);
        if (tap == 0) load_halo(cn, 0);               // next chunk's halo, first half: stored at tap 2 (HALO_FAR: 4)
        if (tap == (HALO_FAR ? 1 : 3)) load_halo(cn, 1);     // second half: stored at tap 5, first read at tap 8
        __builtin_amdgcn_sched_barrier(0);            // keep the loads at the top of the step
        constexpr int nt = tap < 8 ? tap + 1 : 0;
        const int nh = tap < 8 ? hb : hbn;
        auto b0 = [&]() { read_a(q ^ 1, 1, nh, nt); };
        auto b1 = [&]() { read_a(q ^ 1, 0, nh, nt); };
        if constexpr (ring == 0) mfma_step(q, F3_IC(tap / 3), fb0, b0, b1);
        else if constexpr (ring == 1) mfma_step(q, F3_IC(tap / 3), fb1, b0, b1);
        else mfma_step(q, F3_IC(tap / 3), fb2, b0, b1);
        if (tap == (HALO_FAR ? 4 : 2)) store_halo(hbn, 0);
        if (tap == 5) store_halo(hbn, 1);
        // tap 1: every wave is past the previous chunk's tap 7, the last reader of halo buffer cp^1,
        // before anyone overwrites it at tap 2; tap 6: both halves stored before the reads of tap 8
        // (three halo buffers: the one being filled was last read two chunks ago, and the tap-6 barrier bounds the drift
        // of the waves to less than a chunk: the tap-1 barrier is not needed)
        if ((tap == 1 && NHB == 2) || tap == 6) __syncthreads();
    };
    auto chunk_body = [&](auto cp_, int chunk) {
        const int cn = chunk < last ? chunk + 1 : chunk;         // clamped: the last chunk re-reads itself
        const int hb = chunk % NHB, hbn = (chunk + 1) % NHB;
        step(cp_, F3_IC(0), chunk, cn, hb, hbn); step(cp_, F3_IC(1), chunk, cn, hb, hbn); step(cp_, F3_IC(2), chunk, cn, hb, hbn);
        step(cp_, F3_IC(3), chunk, cn, hb, hbn); step(cp_, F3_IC(4), chunk, cn, hb, hbn); step(cp_, F3_IC(5), chunk, cn, hb, hbn);
        step(cp_, F3_IC(6), chunk, cn, hb, hbn); step(cp_, F3_IC(7), chunk, cn, hb, hbn); step(cp_, F3_IC(8), chunk, cn, hb, hbn);
    };
    // (SRC 1: a workgroup whose whole halo is empty has nothing to add to its zero accumulators)
    for (int chunk0 = SRC != 0 && live == 0 ? nchunks : 0; chunk0 < nchunks; chunk0 += 2) {       // nchunks is even (checked by the launcher)
        chunk_body(F3_IC(0), chunk0);
        chunk_body(F3_IC(1), chunk0 + 1);
    }

    if constexpr (IO != 1) {
        // Private to this kernel (not conv2d_tile.h's row epilogue): the scratch is the halo storage and IO = 2 writes pair pixels.
        // Each image row of the wave's tile (32 pixels x 64 channels) goes through a wave-private scratch in the halo
        // storage so that a lane holds 8 consecutive channels of a pixel and stores 32 contiguous bytes with two
        // 16-byte stores (-3 % against one dword per lane and C register straight from the fragment layout; IO = 1
        // keeps that form for A/B).  IO = 2: pair pixels out (sp_rows.h; the consumers are the DMA-fed generic
        // launches, which then skip their split): the lane splits its 8 values once and stores xh[8] | xl'[8].
        __syncthreads();                               // every wave is done reading the halo buffers
        constexpr int SP = 68;
        float* scr = reinterpret_cast<float*>(&Ah[0][0][0]) + wave * (32 * SP);
        static_assert(4 * 32 * SP * 4 <= (int)sizeof(Ah), "scratch must fit the halo storage");
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int y = ty_ * G3_TH + row0 + i;
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const int n = n0 + ch0 + j * 32 + fr;
                const float sc = p.scale[n];
                const float sh = p.shift ? p.shift[n] : 0.0f;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    float v = acc[i][j][r] * sc + sh;
                    if (p.relu) v = v <= 0.f ? 0.f : v;
                    scr[(f3_crow(r, fh)) * SP + j * 32 + fr] = v;
                }
            }
            __builtin_amdgcn_s_waitcnt(0xc07f);
            __builtin_amdgcn_wave_barrier();
            constexpr int GPP = 4 * NJ;                // 8-channel groups per pixel of the wave's row
#pragma unroll
            for (int q = 0; q < 2 * NJ; ++q) {
                const int t = lane + 64 * q, pl = t / GPP, g = t % GPP;
                const int x = tx_ * G3_TW + pl;
                if (y >= p.OH || x >= p.OW) continue;
                const float4 a = *reinterpret_cast<const float4*>(scr + pl * SP + g * 8);
                const float4 b4 = *reinterpret_cast<const float4*>(scr + pl * SP + g * 8 + 4);
                const float v[8] = {a.x, a.y, a.z, a.w, b4.x, b4.y, b4.z, b4.w};
                float* o = p.out + (((int64_t)b * p.OH + y) * p.OW + x) * p.ldc + p.coff + n0 + ch0 + g * 8;
                if constexpr ((IO & SP_IO_OUT_PAIR) != 0) {
                    uint4 hi, lo;
                    sp_split8(v, hi, lo);
                    *reinterpret_cast<uint4*>(o) = hi;
                    *reinterpret_cast<uint4*>(o + 4) = lo;
                } else {
                    *reinterpret_cast<float4*>(o) = a;
                    *reinterpret_cast<float4*>(o + 4) = b4;
                }
            }
            __builtin_amdgcn_wave_barrier();
        }
        return;
    }
    conv_store_rows<G3_TH, G3_TW, NI, NJ, false, false>(p, acc, b, ty_, tx_, row0, n0 + ch0, lane);     // Cout % 128 == 0: no channel test
}

// ------------------------------------------------------------------ 3x3 / stride 1 / pad 1 on v_mfma_f32_16x16x32_f16
// The kernel above is power-limited: its matrix-core instructions toggle enough silicon that the chip drops to
// ~1.64 GHz under it.  On random f16 operands a bare v_mfma_f32_16x16x32_f16 loop sustains 1.93
// PFLOP/s against 1.63 for v_mfma_f32_32x32x16_f16 (tools/probes/mfma_shape_probe.hip) -- the same work at less power.
// This is the same data flow on the narrower shape: a step is (tap, PAIR of 16-channel chunks) = one K=32 MFMA depth,
// the wave tile stays 2 image rows x 32 pixels x 64 channels = 4 x 4 tiles of 16 x 16, the halo of both chunks of a pair
// sits in LDS (double-buffered by pair parity), weights stream from L2 in 16x16x32 fragment order
// ([plane][Cout/16][pair][tap][lane][8], al3d_pack_f16x3_frag16) one step ahead.  The k-blocks of a fragment are
// assigned so that the two lane quarters a b128 read group mixes (q = 0,1 / 2,3) read the SAME 16-byte half of their
// halo rows from the two chunk buffers (bases 256-byte aligned): (3 * pixel + const) mod 16 over 16 distinct pixels ->
// conflict-free at the 48-byte pitch.  Per (pixel, channel) the products are still al*wd, ah*wl, ah*wh into one fp32
// accumulator, but 32 input channels deep per instruction instead of 16: NOT bit-identical to the kernels above
// (same error class; tests compare at fp32 tolerance).
typedef float f32x4 __attribute__((ext_vector_type(4)));
#define G16_HBUF 9984                  // one (chunk, plane) halo buffer: 204 pixels x 48 B, padded to a multiple of 256

__global__ __launch_bounds__(256, 2) void conv3x3_f16x3_frag16_kernel(ConvF3Params p)
{
    __shared__ __attribute__((aligned(256))) unsigned char Ah[2][2][2][G16_HBUF];        // [pair parity][chunk][plane] 78 KB
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int wm = wave & 1, wn = wave >> 1;
    const int lr = lane & 15, lq = lane >> 4;
    int tile, nblk;
    if (!f3_tile_of_block(p.ntiles, p.nblocks, p.xmap, tile, nblk)) return;     // padding block of the last group (uniform)
    int tx_, ty_, b;
    conv_tile_decode(tile, p.tiles_x, p.tiles_y, tx_, ty_, b);
    const int n0 = nblk * F3_BN;
    const int y0 = ty_ * G3_TH - 1, x0 = tx_ * G3_TW - 1;       // image coords of halo (0,0)
    const int npairs = p.Cin / 32;
    const int total = 9 * npairs;
    const float* zero = reinterpret_cast<const float*>(&g_f3_zero16);

    // ---- halo of a chunk pair: 2 x 204 pixels x 4 float4 pieces = 1632 pieces, 8 passes of 256 threads in 4 quarters
    float4 rh[2];
    auto load_halo = [&](int pair, int quarter) {
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int piece = tid + 256 * (2 * quarter + k);
            const int c = piece >= 816 ? 1 : 0, rem = piece - 816 * c;
            const int hp = rem >> 2, q = rem & 3;
            int iy, ix;
            const bool ok = conv_halo_pixel<G3_HW>(p, y0, x0, hp, piece < 1632, iy, ix);
            rh[k] = conv_load4(p, ok, b, iy, ix, (2 * pair + c) * F3_BK + 4 * q, zero);
        }
    };
    auto store_halo = [&](int buf, int quarter) {
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int piece = tid + 256 * (2 * quarter + k);
            if (piece >= 1632) continue;
            const int c = piece >= 816 ? 1 : 0, rem = piece - 816 * c;
            const int hp = rem >> 2, q = rem & 3;
            f16x4 h, l;
            f3_split4(rh[k], h, l);
            const int off = hp * F3_LDB + 8 * q;
            *reinterpret_cast<f16x4*>(&Ah[buf][c][0][off]) = h;
            *reinterpret_cast<f16x4*>(&Ah[buf][c][1][off]) = l;
        }
    };

    // ---- this wave's weight stream: [plane][ntile16][step][lane][8]
    const int NT = p.Cout >> 4;
    const int nt0 = (n0 >> 4) + wn * 4;
    const _Float16* bsrc[2];                          // [plane], tile stride = total * 512 elements
#pragma unroll
    for (int pl = 0; pl < 2; ++pl) bsrc[pl] = p.wgt + ((int64_t)(pl * NT + nt0) * total) * 512 + lane * 8;
    const int64_t bt = (int64_t)total * 512;
    // ONE register set [plane][ntile], rolling: the fragments of 16-channel tile j for step s+1 are requested right
    // after tile j's MFMAs of step s were issued -- a full step (48 MFMAs) between request and use, half the registers
    // of a double set
    f16x8 fb[2][4];
    auto load_b1 = [&](int j, int sidx) {
#pragma unroll
        for (int pl = 0; pl < 2; ++pl)
            fb[pl][j] = *reinterpret_cast<const f16x8*>(bsrc[pl] + j * bt + (int64_t)sidx * 512);
    };

    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[i][j][r] = 0.f;

    // A fragment of m-tile mt (image row 2*wm + (mt >> 1), pixels 16*(mt & 1) + lr): k-block lq = chunk (lq & 1),
    // 16-byte half (lq >> 1) of the pixel's 32-byte f16 row
    const int a_off = (lq & 1) * (2 * G16_HBUF) + ((2 * wm) * G3_HW + lr) * F3_LDB + 16 * (lq >> 1);
    f16x8 fa[2][2][4];                                // [set][plane][mtile]
    auto read_a = [&](int set, int pl, int hbuf, int tap) {
        const int ky = tap / 3, kx = tap % 3;
        const unsigned char* base = &Ah[hbuf][0][pl][0] + a_off;
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
            fa[set][pl][mt] = *reinterpret_cast<const f16x8*>(base + (((mt >> 1) + ky) * G3_HW + 16 * (mt & 1) + kx) * F3_LDB);
    };
    // the three products of f3_mac3 in its order, product-major over the four row tiles of a column tile
    auto mfma_step = [&](int set, int snext, auto&& between0, auto&& between1) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const f16x8 wd = f3_lift_down(fb[0][j]);
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[i][j] = f3_mfma16(fa[set][1][i], wd, acc[i][j]);          // xl' * wd
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[i][j] = f3_mfma16(fa[set][0][i], fb[1][j], acc[i][j]);    // xh * wl
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[i][j] = f3_mfma16(fa[set][0][i], fb[0][j], acc[i][j]);    // xh * wh
            load_b1(j, snext);                        // tile j of the next step into the registers just consumed
            if (j == 0) between0();
            if (j == 1) between1();
        }
    };

    // ---- prologue: halo(pair 0) in LDS, B(0) in flight
    const int last = npairs - 1;
#pragma unroll
    for (int j = 0; j < 4; ++j) load_b1(j, 0);
#pragma unroll
    for (int qd = 0; qd < 4; ++qd) { load_halo(0, qd); store_halo(0, qd); }
    __syncthreads();
    read_a(0, 1, 0, 0);
    read_a(0, 0, 0, 0);

    auto step = [&](auto pp_, auto tap_, int pair, int pn) {
        constexpr int pp = decltype(pp_)::value, tap = decltype(tap_)::value;
        constexpr int q = (pp + tap) & 1;             // A fragment set of this step (9 taps: odd)
        const int s1 = pair * 9 + tap + 1;            // the next step's weights (clamped at the end: harmless re-read)
        if (tap == 0 || tap == 2 || tap == 4 || tap == 6) load_halo(pn, tap >> 1);      // next pair's halo, by quarters
        __builtin_amdgcn_sched_barrier(0);            // keep the loads at the top of the step
        constexpr int nh = tap < 8 ? pp : pp ^ 1, nt = tap < 8 ? tap + 1 : 0;
        auto b0 = [&]() { read_a(q ^ 1, 1, nh, nt); };
        auto b1 = [&]() { read_a(q ^ 1, 0, nh, nt); };
        mfma_step(q, s1 < total ? s1 : total - 1, b0, b1);
        if (tap == 1 || tap == 3 || tap == 5 || tap == 7) store_halo(pp ^ 1, tap >> 1);
        // tap 0: every wave is past the previous pair's tap 7, the last reader of halo buffer pp^1, before anyone
        // overwrites it at tap 1; tap 7: all quarters stored before the reads of tap 8
        if (tap == 0 || tap == 7) __syncthreads();
    };
    auto pair_body = [&](auto pp_, int pair) {
        const int pn = pair < last ? pair + 1 : pair;            // clamped: the last pair re-reads itself
        step(pp_, F3_IC(0), pair, pn); step(pp_, F3_IC(1), pair, pn); step(pp_, F3_IC(2), pair, pn);
        step(pp_, F3_IC(3), pair, pn); step(pp_, F3_IC(4), pair, pn); step(pp_, F3_IC(5), pair, pn);
        step(pp_, F3_IC(6), pair, pn); step(pp_, F3_IC(7), pair, pn); step(pp_, F3_IC(8), pair, pn);
    };
    for (int pair0 = 0; pair0 < npairs; pair0 += 2) {            // npairs is even (checked by the launcher)
        pair_body(F3_IC(0), pair0);
        pair_body(F3_IC(1), pair0 + 1);
    }

    // C fragment of a 16 x 16 tile: lane (lr, lq) holds column lr, rows 4*lq .. 4*lq + 3 (its own epilogue: conv2d_tile.h's are
    // written over 32 x 32 fragments)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int n = n0 + wn * 64 + j * 16 + lr;
        const float sc = p.scale[n];
        const float sh = p.shift ? p.shift[n] : 0.0f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int y = ty_ * G3_TH + 2 * wm + (i >> 1);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int x = tx_ * G3_TW + 16 * (i & 1) + 4 * lq + r;
                if (y >= p.OH || x >= p.OW) continue;
                float v = acc[i][j][r] * sc + sh;
                if (p.relu) v = v <= 0.f ? 0.f : v;                   // NaN propagates, like torch.relu
                p.out[(((int64_t)b * p.OH + y) * p.OW + x) * p.ldc + p.coff + n] = v;
            }
        }
    }
}

// ------------------------------------------------------------------ any geometry, weights from L2
// The generic kernel with the weight half of its staging removed, like the 3x3 kernel above: the
// activation tile (128 pixels x 16 channels per step; no tap reuse to keep a halo for) is still
// split once per workgroup and double-buffered in LDS, but every wave streams its B fragments from
// fragment-ordered weights -- [plane][Cout/32 (zero-padded to 128s)][tap][chunk][lane][8] -- into a
// register ring two steps ahead.  Halves the LDS traffic and the staging work of the stride-2 /
// 1x1 / deconvolution / fused-head launches.  Steps are unrolled by six (LDS buffer parity x ring
// of three) so every buffer and register-set index is a constant; all global loads unconditional.
template <int MODE>
__global__ __launch_bounds__(256, 2) void conv2d_f16x3_bstream_kernel(ConvF3Params p)
{
    __shared__ __attribute__((aligned(16))) unsigned char As[2][2][F3_BM * F3_LDB];   // [buf][plane] 24 KB
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int wm = wave & 1, wn = wave >> 1;
    int tile, nblk;
    if (!f3_tile_of_block(p.ntiles, p.nblocks, p.xmap, tile, nblk)) return;     // padding block of the last group (uniform)
    int tx_, ty_, b;
    conv_tile_decode(tile, p.tiles_x, p.tiles_y, tx_, ty_, b);
    const int n0 = nblk * F3_BN;
    const int taps = MODE == 0 ? p.ksize * p.ksize : 1;
    const int tap0 = MODE == 0 ? 0 : blockIdx.z;
    const int wtaps = MODE == 0 ? taps : 4;
    const int kchunks = p.Cin / F3_BK;
    const int total = taps * kchunks;
    const float* zero = reinterpret_cast<const float*>(&g_f3_zero16);

    // A staging: 128 rows x 16 ch f32 = 512 float4, 2 per thread (row ar and ar + 64)
    const int aq = tid & 3, ar = tid >> 2;
    int py[2], px[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int m = ar + 64 * i;
        py[i] = ty_ * F3_TH + m / F3_TW;
        px[i] = tx_ * F3_TW + m % F3_TW;
    }
    float4 ra[2];
    int ltap = 0, lchunk = 0;                         // cursor of the next A load
    auto load_a = [&]() {
        const int ky = MODE == 0 ? ltap / p.ksize : 0, kx = MODE == 0 ? ltap - ky * p.ksize : 0;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            int iy, ix;
            const bool ok = conv_tap_pixel<MODE>(p, py[i], px[i], ky, kx, iy, ix);
            ra[i] = conv_load4(p, ok, b, iy, ix, lchunk * F3_BK + 4 * aq, zero);
        }
        if (ltap * kchunks + lchunk + 1 < total) { if (++lchunk == kchunks) { lchunk = 0; ++ltap; } }
    };
    auto store_a = [&](int buf) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            f16x4 h, l;
            f3_split4(ra[i], h, l);
            const int off = (ar + 64 * i) * F3_LDB + 8 * aq;
            *reinterpret_cast<f16x4*>(&As[buf][0][off]) = h;
            *reinterpret_cast<f16x4*>(&As[buf][1][off]) = l;
        }
    };
    // B stream of this wave: [plane][ntile][tap][chunk][lane][8]
    const int NTl = (p.Cout + 127) / 128 * 4;
    const int nt0 = (n0 >> 5) + wn * 2;
    const _Float16* bsrc[2][2];
#pragma unroll
    for (int pl = 0; pl < 2; ++pl)
#pragma unroll
        for (int j = 0; j < 2; ++j)
            bsrc[pl][j] = p.wgt + (((int64_t)(pl * NTl + nt0 + j) * wtaps + tap0) * kchunks) * 512 + lane * 8;
    f16x8 fb0[2][2], fb1[2][2], fb2[2][2];
    auto load_b = [&](auto ring_, int sidx) {
        constexpr int ring = decltype(ring_)::value;
        const int sc = sidx < total ? sidx : total - 1;
#pragma unroll
        for (int pl = 0; pl < 2; ++pl)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const f16x8 v = *reinterpret_cast<const f16x8*>(bsrc[pl][j] + (int64_t)sc * 512);
                if constexpr (ring == 0) fb0[pl][j] = v;
                else if constexpr (ring == 1) fb1[pl][j] = v;
                else fb2[pl][j] = v;
            }
    };

    f32x16 acc[2][2];
    conv_acc_clear(acc);

    const int fr = lane & 31, fh = lane >> 5;
    const int a_off = (wm * 64 + fr) * F3_LDB + 16 * fh;
    auto mfma_step = [&](int buf, const f16x8 (&fb)[2][2]) {
        f16x8 a[2][2], wd[2];
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int pl = 0; pl < 2; ++pl)
                a[pl][t] = *reinterpret_cast<const f16x8*>(&As[buf][pl][a_off + t * 32 * F3_LDB]);
#pragma unroll
        for (int j = 0; j < 2; ++j) wd[j] = f3_lift_down(fb[0][j]);
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) f3_mac3(a[0][i], a[1][i], fb[0][j], fb[1][j], wd[j], acc[i][j]);
    };
    // step s: B(s+2) requested, A(s+1) requested, MFMAs of step s, A(s+1) split + stored, barrier
    auto step = [&](auto k_, int s) {
        constexpr int k = decltype(k_)::value;        // s % 6
        load_b(F3_IC((k + 2) % 3), s + 2);
        load_a();
        __builtin_amdgcn_sched_barrier(0);
        if (s < total) {
            if constexpr (k % 3 == 0) mfma_step(k & 1, fb0);
            else if constexpr (k % 3 == 1) mfma_step(k & 1, fb1);
            else mfma_step(k & 1, fb2);
        }
        store_a((k & 1) ^ 1);
        __syncthreads();
    };

    load_a();                                         // A(0)
    load_b(F3_IC(0), 0);
    load_b(F3_IC(1), 1);
    store_a(0);
    __syncthreads();
    for (int s0 = 0; s0 < total; s0 += 6) {
        step(F3_IC(0), s0); step(F3_IC(1), s0 + 1); step(F3_IC(2), s0 + 2);
        step(F3_IC(3), s0 + 3); step(F3_IC(4), s0 + 4); step(F3_IC(5), s0 + 5);
    }

    conv_store_patch<MODE, F3_TH, F3_TW, 2, 2, false, false>(p, acc, b, ty_, tx_, wm, n0 + wn * 64, tap0, lane);
}

// planes [2][Cout][taps][Cin] -> [2][ceil(Cout/128)*4][taps][Cin/16][64][8], zero rows beyond Cout
__global__ void pack_bstream_kernel(const _Float16* __restrict__ planes, int Cout, int taps, int Cin,
                                    _Float16* __restrict__ out, int64_t count)
{
    const int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= count) return;
    const int nchunks = Cin / 16, NTl = (Cout + 127) / 128 * 4;
    int64_t r = o;
    const int e = r % 8; r /= 8;
    const int lane = r % 64; r /= 64;
    const int chunk = r % nchunks; r /= nchunks;
    const int tap = r % taps; r /= taps;
    const int nt = r % NTl; r /= NTl;
    const int pl = (int)r;
    const int n = nt * 32 + (lane & 31), k = chunk * 16 + 8 * (lane >> 5) + e;
    out[o] = n < Cout ? planes[(int64_t)pl * Cout * taps * Cin + ((int64_t)n * taps + tap) * Cin + k] : (_Float16)0.0f;
}

extern "C" int64_t al3d_pack_f16x3_bstream_elems(int Cout, int taps, int Cin)
{
    if (Cout < 1 || taps < 1 || Cin < 16 || Cin % 16) return -1;
    return 2 * (int64_t)((Cout + 127) / 128 * 128) * taps * Cin;
}

extern "C" int al3d_pack_f16x3_bstream(const void* planes_f16x2, int Cout, int taps, int Cin, void* out_frag,
                                       void* stream)
{
    AL3D_REQUIRE(planes_f16x2 && out_frag, "al3d_pack_f16x3_bstream: null pointer");
    const int64_t count = al3d_pack_f16x3_bstream_elems(Cout, taps, Cin);
    AL3D_REQUIRE(count > 0, "al3d_pack_f16x3_bstream: needs Cin %% 16 == 0 (got Cout %d, taps %d, Cin %d)", Cout, taps, Cin);
    hipLaunchKernelGGL(pack_bstream_kernel, dim3((unsigned)al3d_cdiv(count, 256)), dim3(256), 0,
                       (hipStream_t)stream, (const _Float16*)planes_f16x2, Cout, taps, Cin, (_Float16*)out_frag, count);
    AL3D_CHECK_LAUNCH("pack_bstream_kernel");
    return AL3D_OK;
}

// ------------------------------------------------------------------ host side: one parameter builder for every launch
// What a kernel family asks of a launch: its workgroup's pixel tile, whether the kernel strides over two weight planes
// (the fragment-ordered and LDS-image formats of the generic kernels interleave them: plane = 0), and the checks it
// adds to conv_geom_check
struct ConvF3Family {
    int th, tw;
    bool planes;         // p.plane = Cout * taps * Cin
    int cin_mult;        // > 0, the fragment-streamed 3x3 kernels: Cout % 128 == 0 and Cin % cin_mult == 0
    bool dma;            // the LDS-DMA kernel: io flags, 32-bit input offsets
};
static const ConvF3Family F3_FAM_LDS = {F3_TH, F3_TW, true, 0, false}, F3_FAM_HALO = {G3_TH, G3_TW, true, 0, false},
                          F3_FAM_BSTREAM = {F3_TH, F3_TW, false, 0, false}, F3_FAM_FRAG = {G3_TH, G3_TW, true, 32, false},
                          F3_FAM_FRAG16 = {G3_TH, G3_TW, true, 64, false}, F3_FAM_DMA = {F3_TH, F3_TW, false, 0, true};

// Checks the arguments of entry point `name`, fills the parameters and calls launch(p, grid); `kernel` names the launch in
// a launch error.  deconv: the 2x2 / stride-2 transposed conv (pixel tiles over the input map, one grid plane per tap;
// ksize, stride, pad = 2, 2, 0).  gap may be null; io: sp_rows.h flags (LDS-DMA family, 0 elsewhere)
template <class Launch>
static int convf3_launch(const char* name, const char* kernel, const ConvF3Family& fam, const float* in, const void* wgt,
                         const float* scale, const float* shift, float* out, int B, int H, int W, int Cin, int Cout,
                         int ksize, int stride, int pad, bool deconv, int ldc, int coff, int relu, float* gap,
                         int gap_parts, int io, Launch&& launch)
{
    ConvF3Params p;
    p.gap = gap; p.gap_parts = gap_parts; p.io = io;
    p.wgt = (const _Float16*)wgt;
    if (fam.dma) {
        AL3D_REQUIRE(io >= 0 && io < 4 && (!(io & 2) || (Cout % 8 == 0 && ldc % 8 == 0 && coff % 8 == 0)),
                     "%s: bad io flags (pair output needs Cout, ldc, coff multiples of 8)", name);
        AL3D_REQUIRE(io == 0 || (f3_knobs().dma_pipe && f3_knobs().dma_stages == 3),
                     "%s: pair pixels need the shipped kernel shape (AL3D_DMA_PIPE=1, 3 stages)", name);
    }
    int rc = conv_geom_build(p, name, deconv, fam.th, fam.tw, F3_BK, true, in, wgt, scale, shift, out, B, H, W, Cin, Cout, ksize,
                             stride, pad, ldc, coff, relu);
    if (rc) return rc;
    p.plane = fam.planes ? (int64_t)Cout * (deconv ? 4 : ksize * ksize) * Cin : 0;
    AL3D_REQUIRE(!fam.cin_mult || (Cout % 128 == 0 && Cin % fam.cin_mult == 0),
                 "%s: needs Cout %% 128 == 0 and Cin %% %d == 0 (got %d, %d)", name, fam.cin_mult, Cout, Cin);
    AL3D_REQUIRE(!fam.dma || (int64_t)B * H * W * Cin < ((int64_t)1 << 31), "%s: input above 2^31 elements", name);
    AL3D_REQUIRE(!gap || gap_parts >= al3d_gap_parts_count(p.OH, p.OW, deconv),
                 "%s: gap_parts must be at least al3d_gap_parts_count(OH, OW, %d)", name, (int)deconv);
    p.ntiles = p.tiles_x * p.tiles_y * B; p.nblocks = (int)al3d_cdiv(Cout, F3_BN);
    launch(p, deconv ? dim3(f3_grid(p), 1, 4) : dim3(f3_grid(p)));
    AL3D_CHECK_LAUNCH(kernel);
    return AL3D_OK;
}

// f(integral_constant<int, V>) for the first V that equals v, for the last V when none does: one instantiation of f per V
template <int... V, class F> static void f3_switch(int v, F&& f)
{
    constexpr int vals[] = {V...}, last = vals[sizeof...(V) - 1];
    (void)(... || ((v == V || V == last) && (f(F3_IC(V)), true)));
}

extern "C" int al3d_conv2d_nhwc_f16x3_bstream(const float* in, const void* wgt_frag, const float* scale,
                                              const float* shift, float* out, int B, int H, int W, int Cin,
                                              int Cout, int ksize, int stride, int pad, int ldc, int coff,
                                              int relu, void* stream)
{
    return convf3_launch("al3d_conv2d_nhwc_f16x3_bstream", "conv2d_f16x3_bstream_kernel<conv>", F3_FAM_BSTREAM, in, wgt_frag,
                         scale, shift, out, B, H, W, Cin, Cout, ksize, stride, pad, false, ldc, coff, relu, nullptr, 0, 0,
                         [&](const ConvF3Params& p, dim3 grid) {
        hipLaunchKernelGGL(conv2d_f16x3_bstream_kernel<0>, grid, dim3(256), 0, (hipStream_t)stream, p);
    });
}

extern "C" int al3d_deconv2x2_nhwc_f16x3_bstream(const float* in, const void* wgt_frag, const float* scale,
                                                 const float* shift, float* out, int B, int H, int W, int Cin,
                                                 int Cout, int ldc, int coff, int relu, void* stream)
{
    return convf3_launch("al3d_deconv2x2_nhwc_f16x3_bstream", "conv2d_f16x3_bstream_kernel<deconv>", F3_FAM_BSTREAM, in,
                         wgt_frag, scale, shift, out, B, H, W, Cin, Cout, 2, 2, 0, true, ldc, coff, relu, nullptr, 0, 0,
                         [&](const ConvF3Params& p, dim3 grid) {
        hipLaunchKernelGGL(conv2d_f16x3_bstream_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, p);
    });
}

// planes [2][Cout][9][Cin] (al3d_split_f16x3) -> fragment order [2][Cout/32][Cin/16][9][64][8]
__global__ void pack_frag_kernel(const _Float16* __restrict__ planes, int Cout, int Cin, _Float16* __restrict__ out)
{
    const int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t per_plane = (int64_t)Cout * 9 * Cin;
    if (o >= 2 * per_plane) return;
    const int nchunks = Cin / 16;
    int64_t r = o;
    const int e = r % 8; r /= 8;
    const int lane = r % 64; r /= 64;
    const int tap = r % 9; r /= 9;
    const int chunk = r % nchunks; r /= nchunks;
    const int nt = r % (Cout / 32); r /= (Cout / 32);
    const int pl = (int)r;
    const int n = nt * 32 + (lane & 31), k = chunk * 16 + 8 * (lane >> 5) + e;
    out[o] = planes[pl * per_plane + ((int64_t)n * 9 + tap) * Cin + k];
}

extern "C" int al3d_pack_f16x3_frag(const void* planes_f16x2, int Cout, int Cin, void* out_frag, void* stream)
{
    AL3D_REQUIRE(planes_f16x2 && out_frag, "al3d_pack_f16x3_frag: null pointer");
    AL3D_REQUIRE(Cout >= 128 && Cout % 128 == 0 && Cin >= 32 && Cin % 32 == 0,
                 "al3d_pack_f16x3_frag: needs Cout %% 128 == 0 and Cin %% 32 == 0 (got %d, %d)", Cout, Cin);
    const int64_t count = 2 * (int64_t)Cout * 9 * Cin;
    hipLaunchKernelGGL(pack_frag_kernel, dim3((unsigned)al3d_cdiv(count, 256)), dim3(256), 0,
                       (hipStream_t)stream, (const _Float16*)planes_f16x2, Cout, Cin, (_Float16*)out_frag);
    AL3D_CHECK_LAUNCH("pack_frag_kernel");
    return AL3D_OK;
}

// [2][Cout][9][Cin] planes -> 16x16x32 fragment order [plane][Cout/16][pair][tap][lane][8]; lane (c, q) = output channel
// 16*ntile + c, k-block q = input channels 32*pair + 16*(q & 1) + 8*(q >> 1) .. + 7 (conv3x3_f16x3_frag16_kernel)
__global__ void pack_frag16_kernel(const _Float16* __restrict__ planes, int Cout, int Cin, _Float16* __restrict__ out)
{
    const int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t per_plane = (int64_t)Cout * 9 * Cin;
    if (o >= 2 * per_plane) return;
    const int npairs = Cin / 32;
    int64_t r = o;
    const int e = r % 8; r /= 8;
    const int lane = r % 64; r /= 64;
    const int tap = r % 9; r /= 9;
    const int pair = r % npairs; r /= npairs;
    const int nt = r % (Cout / 16); r /= (Cout / 16);
    const int pl = (int)r;
    const int q = lane >> 4;
    const int n = nt * 16 + (lane & 15), k = pair * 32 + 16 * (q & 1) + 8 * (q >> 1) + e;
    out[o] = planes[pl * per_plane + ((int64_t)n * 9 + tap) * Cin + k];
}

extern "C" int al3d_pack_f16x3_frag16(const void* planes_f16x2, int Cout, int Cin, void* out_frag, void* stream)
{
    AL3D_REQUIRE(planes_f16x2 && out_frag, "al3d_pack_f16x3_frag16: null pointer");
    AL3D_REQUIRE(Cout >= 128 && Cout % 128 == 0 && Cin >= 64 && Cin % 64 == 0,
                 "al3d_pack_f16x3_frag16: needs Cout %% 128 == 0 and Cin %% 64 == 0 (got %d, %d)", Cout, Cin);
    const int64_t count = 2 * (int64_t)Cout * 9 * Cin;
    hipLaunchKernelGGL(pack_frag16_kernel, dim3((unsigned)al3d_cdiv(count, 256)), dim3(256), 0,
                       (hipStream_t)stream, (const _Float16*)planes_f16x2, Cout, Cin, (_Float16*)out_frag);
    AL3D_CHECK_LAUNCH("pack_frag16_kernel");
    return AL3D_OK;
}

extern "C" int al3d_conv3x3_nhwc_f16x3_frag16(const float* in, const void* wgt_frag16, const float* scale,
                                              const float* shift, float* out, int B, int H, int W, int Cin,
                                              int Cout, int ldc, int coff, int relu, void* stream)
{
    return convf3_launch("al3d_conv3x3_nhwc_f16x3_frag16", "conv3x3_f16x3_frag16_kernel", F3_FAM_FRAG16, in, wgt_frag16, scale,
                         shift, out, B, H, W, Cin, Cout, 3, 1, 1, false, ldc, coff, relu, nullptr, 0, 0,
                         [&](const ConvF3Params& p, dim3 grid) {
        hipLaunchKernelGGL(conv3x3_f16x3_frag16_kernel, grid, dim3(256), 0, (hipStream_t)stream, p);
    });
}

// Epilogue (first template argument): 2 = pair pixels, 1 = untransposed f32 stores (AL3D_FRAG_EPI=direct, or a window the
// 16-byte stores cannot serve), 0 = 16-byte stores.  Wave shape (second): 2 (default, round 5) = four image rows x ONE
// 32-channel tile per wave, the next chunk's halo halves in their own registers (requested at taps 0 / 1, stored at taps
// 4 / 5); 1 = the same wave shape with the halves sharing two registers (requested at 0 / 3, stored at 2 / 5); 0 = round 1's
// two rows x two tiles (AL3D_FRAG_SHAPE=0|1 for A/B).  Same bits; the nine `<0>` launches of the neck: 1,670 (shape 0) ->
// 1,607 (1) -> 1,597 us (2) on one box
// bev != null: `in` is the sparse rows [n][rows_pitch] of the map and bev its row index (SRC 1; wave shape 2 only)
static int conv3x3_frag_impl(const float* in, const void* wgt_frag, const float* scale, const float* shift, float* out,
                             int B, int H, int W, int Cin, int Cout, int ldc, int coff, int relu, int io, void* stream,
                             const int* bev = nullptr, int rows_pitch = 0)
{
    const bool vec_ok = ldc % 4 == 0 && coff % 4 == 0 && ((uintptr_t)out & 15) == 0;
    const int epi = (io & SP_IO_OUT_PAIR) ? 2 : (f3_knobs().frag_direct || !vec_ok) ? 1 : 0;
    const int shape = f3_knobs().frag_shape == 2 ? 2 : f3_knobs().frag_shape ? 1 : 0;
    return convf3_launch("al3d_conv3x3_nhwc_f16x3_frag", "conv3x3_f16x3_frag_kernel", F3_FAM_FRAG, in, wgt_frag, scale, shift,
                         out, B, H, W, Cin, Cout, 3, 1, 1, false, ldc, coff, relu, nullptr, 0, 0,
                         [&](const ConvF3Params& p, dim3 grid) {
        if (bev) {
            ConvF3Params r = p;
            r.rows = in; r.bev = bev; r.rows_pitch = rows_pitch;
            f3_switch<2, 1, 0>(epi, [&](auto epi_) {
                hipLaunchKernelGGL((conv3x3_f16x3_frag_kernel<decltype(epi_)::value, 2, 1>), grid, dim3(256), 0,
                                   (hipStream_t)stream, r);
            });
            return;
        }
        f3_switch<2, 1, 0>(shape, [&](auto shape_) { f3_switch<2, 1, 0>(epi, [&](auto epi_) {
            hipLaunchKernelGGL((conv3x3_f16x3_frag_kernel<decltype(epi_)::value, decltype(shape_)::value>), grid, dim3(256), 0,
                               (hipStream_t)stream, p);
        }); });
    });
}

extern "C" int al3d_conv3x3_nhwc_f16x3_frag(const float* in, const void* wgt_frag, const float* scale,
                                            const float* shift, float* out, int B, int H, int W, int Cin,
                                            int Cout, int ldc, int coff, int relu, void* stream)
{
    return conv3x3_frag_impl(in, wgt_frag, scale, shift, out, B, H, W, Cin, Cout, ldc, coff, relu, 0, stream);
}

// ... writing pair pixels (io = 2, csrc/sp_rows.h) for a consumer on the LDS-DMA kernel; io = 0: as above
extern "C" int al3d_conv3x3_nhwc_f16x3_frag_io(const float* in, const void* wgt_frag, const float* scale,
                                               const float* shift, float* out, int B, int H, int W, int Cin,
                                               int Cout, int ldc, int coff, int relu, int io, void* stream)
{
    AL3D_REQUIRE(io == 0 || (io == 2 && ldc % 8 == 0 && coff % 8 == 0),
                 "al3d_conv3x3_nhwc_f16x3_frag_io: io must be 0 or 2 (pair output; ldc, coff multiples of 8)");
    return conv3x3_frag_impl(in, wgt_frag, scale, shift, out, B, H, W, Cin, Cout, ldc, coff, relu, io, stream);
}

// ... reading the map from the sparse encoder's last level (D = 2) instead of a dense tensor: rows [n][rows_pitch] f32 and
// their BEV index bev [B,H,W,2] i32 (al3d_sp_bev_index; -1 = no row); map channel c * 2 + z = rows[bev[b][y][x][z]][c],
// Cin = 2 * (channels per row).  The same bits as the call above on the dense map
extern "C" int al3d_conv3x3_nhwc_f16x3_frag_rows(const float* rows, int rows_pitch, const int* bev, const void* wgt_frag,
                                                 const float* scale, const float* shift, float* out, int B, int H, int W,
                                                 int Cin, int Cout, int ldc, int coff, int relu, int io, void* stream)
{
    AL3D_REQUIRE(io == 0 || (io == 2 && ldc % 8 == 0 && coff % 8 == 0),
                 "al3d_conv3x3_nhwc_f16x3_frag_rows: io must be 0 or 2 (pair output; ldc, coff multiples of 8)");
    AL3D_REQUIRE(bev && ((uintptr_t)bev & 7) == 0, "al3d_conv3x3_nhwc_f16x3_frag_rows: bev must be non-null and 8-byte aligned");
    AL3D_REQUIRE(Cin >= 2 && rows_pitch >= Cin / 2 && rows_pitch % 2 == 0,
                 "al3d_conv3x3_nhwc_f16x3_frag_rows: rows_pitch=%d must be even and at least Cin/2=%d", rows_pitch, Cin / 2);
    AL3D_REQUIRE(f3_knobs().frag_shape == 2, "al3d_conv3x3_nhwc_f16x3_frag_rows: built for AL3D_FRAG_SHAPE=2 only");
    return conv3x3_frag_impl(rows, wgt_frag, scale, shift, out, B, H, W, Cin, Cout, ldc, coff, relu, io, stream, bev, rows_pitch);
}

// one-off weight split: f32 [count] * 2^sexp -> f16 [2][count] (wh, wl)
__global__ void split_weights_f16_kernel(const float* __restrict__ w, int64_t count, float mul,
                                         _Float16* __restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const float ws = w[i] * mul;                      // power of two: exact
    const _Float16 wh = (_Float16)ws;
    out[i] = wh;
    out[count + i] = (_Float16)(ws - (float)wh);
}

extern "C" int al3d_split_f16x3(const float* w, int64_t count, int scale_exp, void* out_f16x3, void* stream)
{
    AL3D_REQUIRE(w && out_f16x3 && count >= 0, "al3d_split_f16x3: bad arguments");
    AL3D_REQUIRE(scale_exp >= -100 && scale_exp <= 100, "al3d_split_f16x3: scale exponent %d out of range", scale_exp);
    if (count == 0) return AL3D_OK;
    hipLaunchKernelGGL(split_weights_f16_kernel, dim3((unsigned)al3d_cdiv(count, 256)), dim3(256), 0,
                       (hipStream_t)stream, w, count, ldexpf(1.0f, scale_exp), (_Float16*)out_f16x3);
    AL3D_CHECK_LAUNCH("split_weights_f16_kernel");
    return AL3D_OK;
}


// workgroup partials per image of the fused GAP: pixel tiles of the generic kernel x 2 wave rows (x 4 deconv taps)
extern "C" int al3d_gap_parts_count(int OH, int OW, int deconv)
{
    if (deconv) return (int)(al3d_cdiv(OW / 2, F3_TW) * al3d_cdiv(OH / 2, F3_TH)) * 8;
    return (int)(al3d_cdiv(OW, F3_TW) * al3d_cdiv(OH, F3_TH)) * 2;
}

extern "C" int al3d_gap_reduce_parts_f32(const float* gap_part, int B, int parts, int C, int64_t count, float* out,
                                         void* stream)
{
    AL3D_REQUIRE(gap_part && out && B >= 1 && parts >= 1 && C >= 1 && count >= 1, "al3d_gap_reduce_parts_f32: bad arguments");
    hipLaunchKernelGGL(gap_parts_reduce_kernel, dim3((unsigned)al3d_cdiv(C, 64), (unsigned)B), dim3(64), 0,
                       (hipStream_t)stream, gap_part, parts, C, (float)count, out);
    AL3D_CHECK_LAUNCH("gap_parts_reduce_kernel");
    return AL3D_OK;
}

static int conv2d_f16x3_impl(const char* name, const float* in, const void* wgt_f16x3, const float* scale,
                             const float* shift, float* out, int B, int H, int W, int Cin,
                             int Cout, int ksize, int stride, int pad, int ldc, int coff,
                             int relu, float* gap_part, int gap_parts, void* stream)
{
    // halo-staged fast path (chunk pairs): 3x3/s1/p1 without the fused GAP
    const bool halo = !gap_part && ksize == 3 && stride == 1 && pad == 1 && Cin % (2 * F3_BK) == 0;
    return convf3_launch(name, halo ? "conv3x3_f16x3_halo_kernel" : "conv2d_f16x3_kernel<conv>", halo ? F3_FAM_HALO : F3_FAM_LDS,
                         in, wgt_f16x3, scale, shift, out, B, H, W, Cin, Cout, ksize, stride, pad, false, ldc, coff, relu,
                         gap_part, gap_parts, 0, [&](const ConvF3Params& p, dim3 grid) {
        if (halo) hipLaunchKernelGGL(conv3x3_f16x3_halo_kernel, grid, dim3(256), 0, (hipStream_t)stream, p);
        else hipLaunchKernelGGL(conv2d_f16x3_kernel<0>, grid, dim3(256), 0, (hipStream_t)stream, p);
    });
}

extern "C" int al3d_conv2d_nhwc_f16x3(const float* in, const void* wgt_f16x3, const float* scale,
                                      const float* shift, float* out, int B, int H, int W, int Cin,
                                      int Cout, int ksize, int stride, int pad, int ldc, int coff,
                                      int relu, void* stream)
{
    return conv2d_f16x3_impl("al3d_conv2d_nhwc_f16x3", in, wgt_f16x3, scale, shift, out, B, H, W, Cin, Cout, ksize, stride, pad,
                             ldc, coff, relu, nullptr, 0, stream);
}

extern "C" int al3d_conv2d_nhwc_f16x3_gap(const float* in, const void* wgt_f16x3, const float* scale,
                                          const float* shift, float* out, int B, int H, int W, int Cin,
                                          int Cout, int ksize, int stride, int pad, int ldc, int coff,
                                          int relu, float* gap_part, int gap_parts, void* stream)
{
    AL3D_REQUIRE(gap_part, "al3d_conv2d_nhwc_f16x3_gap: null gap_part");
    return conv2d_f16x3_impl("al3d_conv2d_nhwc_f16x3_gap", in, wgt_f16x3, scale, shift, out, B, H, W, Cin, Cout, ksize, stride,
                             pad, ldc, coff, relu, gap_part, gap_parts, stream);
}

static int deconv2x2_f16x3_impl(const char* name, const float* in, const void* wgt_f16x3, const float* scale,
                                const float* shift, float* out, int B, int H, int W, int Cin,
                                int Cout, int ldc, int coff, int relu, float* gap_part, int gap_parts, void* stream)
{
    return convf3_launch(name, "conv2d_f16x3_kernel<deconv>", F3_FAM_LDS, in, wgt_f16x3, scale, shift, out, B, H, W, Cin, Cout,
                         2, 2, 0, true, ldc, coff, relu, gap_part, gap_parts, 0, [&](const ConvF3Params& p, dim3 grid) {
        hipLaunchKernelGGL(conv2d_f16x3_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, p);
    });
}

extern "C" int al3d_deconv2x2_nhwc_f16x3(const float* in, const void* wgt_f16x3, const float* scale,
                                         const float* shift, float* out, int B, int H, int W, int Cin,
                                         int Cout, int ldc, int coff, int relu, void* stream)
{
    return deconv2x2_f16x3_impl("al3d_deconv2x2_nhwc_f16x3", in, wgt_f16x3, scale, shift, out, B, H, W, Cin, Cout, ldc, coff,
                                relu, nullptr, 0, stream);
}

extern "C" int al3d_deconv2x2_nhwc_f16x3_gap(const float* in, const void* wgt_f16x3, const float* scale,
                                             const float* shift, float* out, int B, int H, int W, int Cin,
                                             int Cout, int ldc, int coff, int relu, float* gap_part, int gap_parts,
                                             void* stream)
{
    AL3D_REQUIRE(gap_part, "al3d_deconv2x2_nhwc_f16x3_gap: null gap_part");
    return deconv2x2_f16x3_impl("al3d_deconv2x2_nhwc_f16x3_gap", in, wgt_f16x3, scale, shift, out, B, H, W, Cin, Cout, ldc,
                                coff, relu, gap_part, gap_parts, stream);
}

// ------------------------------------------------------------------ any geometry, both operands by LDS-DMA
// The generic kernels above move every operand through registers on its way to LDS (global load -> split ->
// ds_write) and wait at a barrier for the slowest of 256 such round trips once per 16-channel step; the
// streamed-weight variant trades the weight half of that for four fragment loads per wave and step, which the
// texture-address unit serves at 64 B/clk -- as many cycles as the step's twelve MFMAs.  Profiled, the stride-2,
// 1x1, deconvolution and fused-head launches sat at 180-240 TFLOP/s of products against 350 for the 3x3 kernel.
//
// Here nothing passes through a register before it is an MFMA operand.  A step's two tiles -- 128 pixels x 16
// channels of RAW fp32 activations (8 KB) and 128 output channels x 16 x {wh, wl} f16 weights (8 KB, an image
// pre-packed in exactly the LDS layout) -- are fetched by `global_load_lds_dwordx4`, four DMA instructions per
// wave and step, into a ring of NS stages that runs NS-1 steps ahead; counted `s_waitcnt vmcnt` + ONE raw
// `s_barrier` per step publish a stage.  The activation split (xh, xl') happens on the fragment, in registers,
// after the ds_read -- 2 x more VALU than splitting once per workgroup, but off the critical path of the loads.
// The stage layout, the source-side swizzle, the fragment offsets and reads, and the pipelined loop of the default
// kernel are al3d_f16x3.h's (f3_ring_gemm, shared with the token GEMM of tokens.hip); this file keeps the pixel / tap
// address generation and the epilogues.
// Same tiles, same grid, same product order as conv2d_f16x3_kernel: bit-identical results, same GAP partials.
__device__ __attribute__((aligned(256))) float g_dma_zero[64];     // stays zero: source of out-of-image pixels

template <int MODE, int NS>
__global__ __launch_bounds__(256, NS <= 3 ? 3 : 2) void conv2d_f16x3_dma_kernel(ConvF3Params p)
{
    __shared__ __attribute__((aligned(1024))) unsigned char smem[NS * F3_RING_STAGE];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave & 1, wn = wave >> 1;
    int tile, nblk;
    if (!f3_tile_of_block(p.ntiles, p.nblocks, p.xmap, tile, nblk)) return;     // padding block of the last group (uniform)
    int tx_, ty_, b;
    conv_tile_decode(tile, p.tiles_x, p.tiles_y, tx_, ty_, b);
    const int n0 = nblk * F3_BN;
    const int taps = MODE == 0 ? p.ksize * p.ksize : 1;
    const int tap0 = MODE == 0 ? 0 : blockIdx.z;
    const int wtaps = MODE == 0 ? taps : 4;
    const int kchunks = p.Cin / F3_BK;
    const int total = taps * kchunks;
    const unsigned smem_base = (unsigned)(size_t)(lds_void*)smem;

    // ---- DMA side.  Wave w fetches M-tile w (pixels 32w .. 32w+31 of the 8 x 16 tile) and the 2 KB quarter w of the
    // weight tile.  Lane (jg, sg) of piece i fetches chunk sg ^ f(r) of row r = 2 jg + i.
    const int jg = lane >> 2, sg = lane & 3;
    int py[2], px[2], cg[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int r = 2 * jg + i, m = 32 * wave + r;
        py[i] = ty_ * F3_TH + m / F3_TW;
        px[i] = tx_ * F3_TW + m % F3_TW;
        cg[i] = (sg ^ f3_ring_swz(r)) * 4;
    }
    const char* wsrc = reinterpret_cast<const char*>(p.wgt) +
                       ((int64_t)nblk * wtaps + tap0) * kchunks * 8192 + wave * 2048 + lane * 16;
    int ltap = 0, lchunk = 0;                          // cursor of the next stage to request
    auto issue = [&](int stage) {
        const int ky = MODE == 0 ? ltap / p.ksize : 0, kx = MODE == 0 ? ltap - ky * p.ksize : 0;
        const unsigned dst = __builtin_amdgcn_readfirstlane(smem_base + stage * F3_RING_STAGE + wave * 2048);
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            int iy, ix;
            const bool ok = conv_tap_pixel<MODE>(p, py[i], px[i], ky, kx, iy, ix);
            // 32-bit element index (the entry checks B*H*W*Cin < 2^31): keeps the select a pair of v_cndmask, no branch
            const unsigned idx = (unsigned)(((b * p.H + iy) * p.W + ix) * p.Cin + lchunk * F3_BK + cg[i]);
            const float* src = ok ? p.in + idx : g_dma_zero + cg[i];
            __builtin_amdgcn_global_load_lds((gbl_void*)src, (lds_void*)(size_t)(dst + i * 1024), 16, 0, 0);
        }
        const char* ws = wsrc + ((int64_t)ltap * kchunks + lchunk) * 8192;
#pragma unroll
        for (int i = 0; i < 2; ++i)
            __builtin_amdgcn_global_load_lds((gbl_void*)(ws + i * 1024), (lds_void*)(size_t)(dst + F3_RING_BOFF + i * 1024),
                                             16, 0, 0);
        // steps past the end re-fetch the last one (into a free stage): the DMA count per step stays 4
        if (ltap * kchunks + lchunk + 1 < total) { if (++lchunk == kchunks) { lchunk = 0; ++ltap; } }
    };

    f32x16 acc[2][2];
    conv_acc_clear(acc);

    const int fr = lane & 31, fh = lane >> 5;
    const F3RingOffs off = f3_ring_offsets(wm, wn, fr, fh);            // fragment side

#pragma unroll
    for (int s = 0; s < NS - 1; ++s) issue(s);
    int stage = 0, fill = NS - 1;
    for (int s = 0; s < total; ++s) {
        f3_wait_vm<4 * (NS - 2)>();                    // this wave's share of stage s has landed ...
        __builtin_amdgcn_s_barrier();                  // ... everyone's has, and stage s-1 is free
        issue(fill);
        f32x4 a0l, a0h, a1l, a1h;
        f16x8 wh[2], wl[2];
        f3_ring_read(a0l, a0h, a1l, a1h, wh[0], wl[0], wh[1], wl[1], smem_base + stage * F3_RING_STAGE, off);
        f16x8 ah[2], al[2];
        f3_split8(a0l, a0h, ah[0], al[0]);
        f3_split8(a1l, a1h, ah[1], al[1]);
        const f16x8 wd[2] = {f3_lift_down(wh[0]), f3_lift_down(wh[1])};
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) f3_mac3(ah[i], al[i], wh[j], wl[j], wd[j], acc[i][j]);
        stage = stage + 1 == NS ? 0 : stage + 1;
        fill = fill + 1 == NS ? 0 : fill + 1;
    }
    f3_wait_vm<0>();                                   // the tail's dummy requests must not outlive the workgroup's LDS

    // same tiles and partials as conv2d_f16x3_kernel
    conv_store_patch<MODE, F3_TH, F3_TW, 2, 2, false, true>(p, acc, b, ty_, tx_, wm, n0 + wn * 64, tap0, lane, p.gap, p.gap_parts);
}

// Software-pipelined form of the kernel above (the default): the loop is f3_ring_gemm (al3d_f16x3.h), all NS stages in
// flight; each accumulator still receives xl'*wd, xh*wl, xh*wh in that order per step: the same bits.
template <int MODE, int NS, int IO = 0>
__global__ __launch_bounds__(256, 2) void conv2d_f16x3_dma2_kernel(ConvF3Params p)
{
    __shared__ __attribute__((aligned(1024))) unsigned char smem[NS * F3_RING_STAGE];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave & 1, wn = wave >> 1;
    int tile, nblk;
    if (!f3_tile_of_block(p.ntiles, p.nblocks, p.xmap, tile, nblk)) return;     // padding block of the last group (uniform)
    int tx_, ty_, b;
    conv_tile_decode(tile, p.tiles_x, p.tiles_y, tx_, ty_, b);
    const int n0 = nblk * F3_BN;
    const int taps = MODE == 0 ? p.ksize * p.ksize : 1;
    const int tap0 = MODE == 0 ? 0 : blockIdx.z;
    const int wtaps = MODE == 0 ? taps : 4;
    const int kchunks = p.Cin / F3_BK;
    const int total = taps * kchunks;
    const unsigned smem_base = (unsigned)(size_t)(lds_void*)smem;

    const int jg = lane >> 2, sg = lane & 3;
    int py[2], px[2], cg[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int r = 2 * jg + i, m = 32 * wave + r;
        py[i] = ty_ * F3_TH + m / F3_TW;
        px[i] = tx_ * F3_TW + m % F3_TW;
        cg[i] = (sg ^ f3_ring_swz(r)) * 4;
    }
    const char* wsrc = reinterpret_cast<const char*>(p.wgt) +
                       ((int64_t)nblk * wtaps + tap0) * kchunks * 8192 + wave * 2048 + lane * 16;
    int ltap = 0, lchunk = 0;                          // cursor of the next stage to request
    // the pixel part of a lane's two source addresses changes only with the tap: recomputed when a tap starts
    // (wave-uniform branch), then one 64-bit multiply-add per request.  Out-of-image pixels: zero row, stride 0.
    const char* abase[2];
    unsigned ainc[2];
    auto issue = [&](int stage) {
        if (lchunk == 0) {
            const int ky = MODE == 0 ? ltap / p.ksize : 0, kx = MODE == 0 ? ltap - ky * p.ksize : 0;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                int iy, ix;
                const bool ok = conv_tap_pixel<MODE>(p, py[i], px[i], ky, kx, iy, ix);
                // 32-bit element index (the entry checks B*H*W*Cin < 2^31)
                const unsigned idx = (unsigned)(((b * p.H + iy) * p.W + ix) * p.Cin + cg[i]);
                abase[i] = reinterpret_cast<const char*>(ok ? p.in + idx : g_dma_zero + cg[i]);
                ainc[i] = ok ? 4u * F3_BK : 0u;
            }
        }
        const unsigned dst = __builtin_amdgcn_readfirstlane(smem_base + stage * F3_RING_STAGE + wave * 2048);
#pragma unroll
        for (int i = 0; i < 2; ++i)
            __builtin_amdgcn_global_load_lds((gbl_void*)(abase[i] + (size_t)lchunk * ainc[i]),
                                             (lds_void*)(size_t)(dst + i * 1024), 16, 0, 0);
        const char* ws = wsrc + ((int64_t)ltap * kchunks + lchunk) * 8192;
#pragma unroll
        for (int i = 0; i < 2; ++i)
            __builtin_amdgcn_global_load_lds((gbl_void*)(ws + i * 1024), (lds_void*)(size_t)(dst + F3_RING_BOFF + i * 1024),
                                             16, 0, 0);
        // steps past the end re-fetch the last one (into a free stage): the DMA count per step stays 4
        if (ltap * kchunks + lchunk + 1 < total) { if (++lchunk == kchunks) { lchunk = 0; ++ltap; } }
    };

#pragma unroll
    for (int s = 0; s < NS; ++s) issue(s);             // fill the ring
    f32x16 c00, c01, c10, c11;
    // row formats are compile-time: no branch in the loop.  Pair pixels in: the 32 bytes of a fragment ARE (xh[8], xl'[8])
    f3_ring_gemm<NS, (IO & SP_IO_IN_PAIR) != 0, f3_split>(smem_base, total, wm, wn, lane, issue, c00, c01, c10, c11);
    const int fr = lane & 31, fh = lane >> 5;

    if constexpr ((IO & 4) == 0) {
        const f32x16* accp[2][2] = {{&c00, &c01}, {&c10, &c11}};
        const int MH = MODE == 0 ? p.OH : p.H, MW = MODE == 0 ? p.OW : p.W;
        // Private to this kernel: the transposition goes through the stage ring, the GAP sums are taken before the store test.
        // BN / ReLU / GAP sums in the C layout, then each 32-pixel x 64-channel half of the wave's tile goes through a
        // wave-private LDS scratch (the stage ring, free after the barrier) so that a lane holds consecutive channels of
        // a pixel and stores 16-byte pieces (IO & 4: the untransposed dword stores below, for layouts that are not
        // 16-byte aligned).  Pair pixels out (IO & 2, sp_rows.h): 8 channels per lane, split once, xh[8] | xl'[8]
        __syncthreads();                               // every wave is done reading the stage ring
        constexpr int SP = 68;                         // floats per scratch row (64 + 4: conflict-free b128 reads)
        float* scr = reinterpret_cast<float*>(smem) + wave * (32 * SP);
        float gs[2] = {0.f, 0.f};
#pragma unroll
        for (int i = 0; i < 2; ++i) {
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int n = n0 + wn * 64 + j * 32 + fr;
                const bool nok = n < p.Cout;
                const float sc = nok ? p.scale[n] : 0.f;
                const float sh = (nok && p.shift) ? p.shift[n] : 0.0f;
                const f32x16& acc = *accp[i][j];
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int ml = f3_crow(r, fh);
                    const int m = wm * 64 + i * 32 + ml;
                    const int y = ty_ * F3_TH + m / F3_TW, x = tx_ * F3_TW + m % F3_TW;
                    float v = acc[r] * sc + sh;
                    if (p.relu) v = v <= 0.f ? 0.f : v;
                    scr[ml * SP + j * 32 + fr] = v;
                    if (y < MH && x < MW) gs[j] += v;
                }
            }
            __builtin_amdgcn_s_waitcnt(0xc07f);
            __builtin_amdgcn_wave_barrier();
            if constexpr ((IO & SP_IO_OUT_PAIR) != 0) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int t = lane + 64 * q, pl = t >> 3, g = t & 7;
                    const int m = wm * 64 + i * 32 + pl;
                    const int y = ty_ * F3_TH + m / F3_TW, x = tx_ * F3_TW + m % F3_TW;
                    const int n = n0 + wn * 64 + g * 8;
                    if (y >= MH || x >= MW || n >= p.Cout) continue;
                    const float4 a = *reinterpret_cast<const float4*>(scr + pl * SP + g * 8);
                    const float4 b4 = *reinterpret_cast<const float4*>(scr + pl * SP + g * 8 + 4);
                    const float v[8] = {a.x, a.y, a.z, a.w, b4.x, b4.y, b4.z, b4.w};
                    uint4 hi, lo;
                    sp_split8(v, hi, lo);
                    int oy = y, ox = x;
                    if (MODE == 1) { oy = 2 * y + (tap0 >> 1); ox = 2 * x + (tap0 & 1); }
                    float* o = p.out + (((int64_t)b * p.OH + oy) * p.OW + ox) * p.ldc + p.coff + n;
                    *reinterpret_cast<uint4*>(o) = hi;
                    *reinterpret_cast<uint4*>(o + 4) = lo;
                }
            } else {
#pragma unroll
                for (int q = 0; q < 8; ++q) {            // f32 pixels: one float4 per lane and trip (Cout % 4 == 0)
                    const int t = lane + 64 * q, pl = t >> 4, g = t & 15;
                    const int m = wm * 64 + i * 32 + pl;
                    const int y = ty_ * F3_TH + m / F3_TW, x = tx_ * F3_TW + m % F3_TW;
                    const int n = n0 + wn * 64 + g * 4;
                    if (y >= MH || x >= MW || n >= p.Cout) continue;
                    int oy = y, ox = x;
                    if (MODE == 1) { oy = 2 * y + (tap0 >> 1); ox = 2 * x + (tap0 & 1); }
                    *reinterpret_cast<float4*>(p.out + (((int64_t)b * p.OH + oy) * p.OW + ox) * p.ldc + p.coff + n) =
                        *reinterpret_cast<const float4*>(scr + pl * SP + g * 4);
                }
            }
            __builtin_amdgcn_wave_barrier();
        }
        if (p.gap) {
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int n = n0 + wn * 64 + j * 32 + fr;
                float gsum = gs[j];
                gsum += __shfl_xor(gsum, 32);
                if (fh == 0 && n < p.Cout) {
                    const int part = (((ty_ * p.tiles_x + tx_) * (MODE == 1 ? 4 : 1) + tap0) << 1) + wm;
                    p.gap[((int64_t)b * p.gap_parts + part) * p.ldc + p.coff + n] = gsum;
                }
            }
        }
        return;
    }
    const f32x16 acc[2][2] = {{c00, c01}, {c10, c11}};
    conv_store_patch<MODE, F3_TH, F3_TW, 2, 2, false, true>(p, acc, b, ty_, tx_, wm, n0 + wn * 64, tap0, lane, p.gap, p.gap_parts);
}

// planes [2][Cout][taps][Cin] -> [ceil(Cout/128)][taps][Cin/16][2 planes][128 rows][2 chunks of 8 f16]; chunk c of
// row n sits at position c ^ ((n >> 3) & 1); rows >= Cout zero.  One (block, tap, chunk) = the 8 KB a stage holds.
__global__ void pack_dma_kernel(const _Float16* __restrict__ planes, int Cout, int taps, int Cin,
                                _Float16* __restrict__ out, int64_t count)
{
    const int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= count) return;
    const int nchunks = Cin / 16;
    int64_t r = o;
    const int e = r % 8; r /= 8;
    const int pos = r % 2; r /= 2;
    const int nl = r % 128; r /= 128;
    const int pl = r % 2; r /= 2;
    const int chunk = r % nchunks; r /= nchunks;
    const int tap = r % taps; r /= taps;
    const int n = (int)r * 128 + nl;
    const int c = pos ^ ((nl >> 3) & 1);
    out[o] = n < Cout ? planes[(int64_t)pl * Cout * taps * Cin + ((int64_t)n * taps + tap) * Cin + chunk * 16 + 8 * c + e]
                      : (_Float16)0.0f;
}

extern "C" int al3d_pack_f16x3_dma(const void* planes_f16x2, int Cout, int taps, int Cin, void* out_image, void* stream)
{
    AL3D_REQUIRE(planes_f16x2 && out_image, "al3d_pack_f16x3_dma: null pointer");
    const int64_t count = al3d_pack_f16x3_bstream_elems(Cout, taps, Cin);     // same size: whole 128-row blocks
    AL3D_REQUIRE(count > 0, "al3d_pack_f16x3_dma: needs Cin %% 16 == 0 (got Cout %d, taps %d, Cin %d)", Cout, taps, Cin);
    hipLaunchKernelGGL(pack_dma_kernel, dim3((unsigned)al3d_cdiv(count, 256)), dim3(256), 0, (hipStream_t)stream,
                       (const _Float16*)planes_f16x2, Cout, taps, Cin, (_Float16*)out_image, count);
    AL3D_CHECK_LAUNCH("pack_dma_kernel");
    return AL3D_OK;
}

// Epilogue form: 16-byte stores through an LDS transposition need Cout, ldc, coff multiples of 4 and an aligned base; else
// (or AL3D_DMA_EPI=direct, for A/B) untransposed dword stores.  The shipped shape (AL3D_DMA_PIPE=1, 3 stages) has all row /
// pixel format combinations; the others f32 pixels and dword stores only
template <int MODE> static void launch_dma(const ConvF3Params& p, dim3 grid, hipStream_t s)
{
    const F3Knobs& k = f3_knobs();
    const bool vec_ok = p.Cout % 4 == 0 && p.ldc % 4 == 0 && p.coff % 4 == 0 && ((uintptr_t)p.out & 15) == 0;
    if (k.dma_pipe && k.dma_stages == 3)
        f3_switch<0, 1, 2, 3, 4, 5>(p.io | ((p.io & 2) == 0 && (k.dma_direct || !vec_ok) ? 4 : 0), [&](auto io_) {
            hipLaunchKernelGGL((conv2d_f16x3_dma2_kernel<MODE, 3, decltype(io_)::value>), grid, dim3(256), 0, s, p);
        });
    else if (k.dma_pipe)
        f3_switch<5, 4>(k.dma_stages, [&](auto ns_) {
            hipLaunchKernelGGL((conv2d_f16x3_dma2_kernel<MODE, decltype(ns_)::value, 4>), grid, dim3(256), 0, s, p);
        });
    else
        f3_switch<4, 5, 3>(k.dma_stages, [&](auto ns_) {
            hipLaunchKernelGGL((conv2d_f16x3_dma_kernel<MODE, decltype(ns_)::value>), grid, dim3(256), 0, s, p);
        });
}

// gap_part may be null (no fused GAP); otherwise [B][gap_parts][ldc] with gap_parts >= al3d_gap_parts_count
extern "C" int al3d_conv2d_nhwc_f16x3_dma(const float* in, const void* wgt_image, const float* scale,
                                          const float* shift, float* out, int B, int H, int W, int Cin,
                                          int Cout, int ksize, int stride, int pad, int ldc, int coff,
                                          int relu, float* gap_part, int gap_parts, int io, void* stream)
{
    return convf3_launch("al3d_conv2d_nhwc_f16x3_dma", "conv2d_f16x3_dma_kernel<conv>", F3_FAM_DMA, in, wgt_image, scale, shift,
                         out, B, H, W, Cin, Cout, ksize, stride, pad, false, ldc, coff, relu, gap_part, gap_parts, io,
                         [&](const ConvF3Params& p, dim3 grid) { launch_dma<0>(p, grid, (hipStream_t)stream); });
}

extern "C" int al3d_deconv2x2_nhwc_f16x3_dma(const float* in, const void* wgt_image, const float* scale,
                                             const float* shift, float* out, int B, int H, int W, int Cin,
                                             int Cout, int ldc, int coff, int relu, float* gap_part, int gap_parts,
                                             int io, void* stream)
{
    return convf3_launch("al3d_deconv2x2_nhwc_f16x3_dma", "conv2d_f16x3_dma_kernel<deconv>", F3_FAM_DMA, in, wgt_image, scale,
                         shift, out, B, H, W, Cin, Cout, 2, 2, 0, true, ldc, coff, relu, gap_part, gap_parts, io,
                         [&](const ConvF3Params& p, dim3 grid) { launch_dma<1>(p, grid, (hipStream_t)stream); });
}
