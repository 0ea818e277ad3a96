// The single header of the f16x3 sparse-convolution kernels (spconv_wave.hip, spconv_glds.hip, spconv_rng.hip,
// spconv_blk.hip, spconv_l0.hip).  Device side (the arithmetic itself is al3d_f16x3.h's): the
// pipelined unit (the three products of a unit in their one summation order), raw LDS reads fused with their waits,
// LDS-DMA piece loops, the XCD placement.  Host side: the argument checks and the launch of every entry point.
#pragma once
#include "al3d_common.h"
#include "sp_rows.h"
#include <stdlib.h>

typedef int gl_i32x4 __attribute__((ext_vector_type(4)));       // native vectors: inline-asm register operands
typedef int gl_i32x2 __attribute__((ext_vector_type(2)));

static __device__ __attribute__((aligned(256))) float g_glds_zero[128];     // stays zero: source of masked gathers
static __device__ __attribute__((aligned(256))) int g_glds_neg1[64] = {      // "no neighbour": index source of items past the end
    -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1,
    -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1};

template <int I> struct gl_int { static constexpr int value = I; };
template <int N, int I = 0, class F> __device__ __forceinline__ void gl_static_for(F&& f)
{
    if constexpr (I < N) {
        f(gl_int<I>{});
        gl_static_for<N, I + 1>(f);
    }
}

// ---- XCD-aware placement: workgroups with equal blockIdx.x % 8 share an L2, so each of the eight groups gets one
// contiguous range of slots (rows are in raster order: the neighbours of a tile live in nearby tiles) instead of every
// eighth one.  Bijective for any grid size.  A kernel multiplies the slot by the tiles (rows, chunks) of its workgroup.
__device__ __forceinline__ int gl_xcd_slot()
{
    const int nwg = gridDim.x, xcd = blockIdx.x & 7, q8 = nwg >> 3, r8 = nwg & 7;
    return (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (blockIdx.x >> 3);
}

// ---- the f16x3 arithmetic is al3d_f16x3.h's (through sp_rows.h): the pair-wise split f3_split8p, f3_lift_down, and the
// three products of a unit SMALLEST FIRST -- al * wd, ah * wl, ah * wh (f3_mac3) -- into one fp32 accumulator, units in
// tap, channel-unit order: every structure keeps this order (gl_read_next_mfma below and the kernels' own triples),
// which is why they all give the same bits.
__device__ __forceinline__ f32x16 gl_zero()                           // a zeroed accumulator tile
{
    f32x16 z;
#pragma unroll
    for (int e = 0; e < 16; ++e) z[e] = 0.f;
    return z;
}

// ---- raw instructions the compiler must not reason about.  Every LDS read of the main loop is ONE asm block
// that also contains its `s_waitcnt lgkmcnt(0)`: with the wait in a separate statement hipcc is free to copy a
// destination register between the two (it did, merging the two arms of a branch) -- before the data arrived.
__device__ __forceinline__ void gl_lds_read_idx(gl_i32x4& d, unsigned addr)
{
    asm volatile("ds_read_b128 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=&v"(d) : "v"(addr) : "memory");
}
__device__ __forceinline__ void gl_lds_read_idx(gl_i32x2& d, unsigned addr)
{
    asm volatile("ds_read_b64 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=&v"(d) : "v"(addr) : "memory");
}
// A fragment only (the B fragments of this (tap, chunk) are already in registers)
__device__ __forceinline__ void gl_lds_read_a(f32x4& lo, f32x4& hi, unsigned a0, unsigned a1)
{
    asm volatile("ds_read_b128 %0, %2\n\tds_read_b128 %1, %3\n\ts_waitcnt lgkmcnt(0)"
                 : "=&v"(lo), "=&v"(hi) : "v"(a0), "v"(a1) : "memory");
}
// A fragment + the B fragments (wh, wl planes) of TN 32-column tiles; OFF = byte offset of the unit in the slab,
// PL = byte distance of the two planes, 32 rows of a plane = 1 KiB
template <int TN, int OFF, int PL>
__device__ __forceinline__ void gl_lds_read_ab(f32x4& lo, f32x4& hi, f16x8 (&wh)[TN], f16x8 (&wl)[TN], unsigned a0,
                                               unsigned a1, unsigned b)
{
    static_assert(TN == 1 || TN == 2 || TN == 4, "tile counts of the supported channel pairs");
    if constexpr (TN == 1)
        asm volatile("ds_read_b128 %0, %4\n\tds_read_b128 %1, %5\n\t"
                     "ds_read_b128 %2, %6 offset:%7\n\tds_read_b128 %3, %6 offset:%8\n\ts_waitcnt lgkmcnt(0)"
                     : "=&v"(lo), "=&v"(hi), "=&v"(wh[0]), "=&v"(wl[0])
                     : "v"(a0), "v"(a1), "v"(b), "n"(OFF), "n"(OFF + PL) : "memory");
    else if constexpr (TN == 2)
        asm volatile("ds_read_b128 %0, %6\n\tds_read_b128 %1, %7\n\t"
                     "ds_read_b128 %2, %8 offset:%9\n\tds_read_b128 %3, %8 offset:%10\n\t"
                     "ds_read_b128 %4, %8 offset:%11\n\tds_read_b128 %5, %8 offset:%12\n\ts_waitcnt lgkmcnt(0)"
                     : "=&v"(lo), "=&v"(hi), "=&v"(wh[0]), "=&v"(wl[0]), "=&v"(wh[1]), "=&v"(wl[1])
                     : "v"(a0), "v"(a1), "v"(b), "n"(OFF), "n"(OFF + PL), "n"(OFF + 1024), "n"(OFF + PL + 1024) : "memory");
    else
        asm volatile("ds_read_b128 %0, %10\n\tds_read_b128 %1, %11\n\t"
                     "ds_read_b128 %2, %12 offset:%13\n\tds_read_b128 %3, %12 offset:%14\n\t"
                     "ds_read_b128 %4, %12 offset:%15\n\tds_read_b128 %5, %12 offset:%16\n\t"
                     "ds_read_b128 %6, %12 offset:%17\n\tds_read_b128 %7, %12 offset:%18\n\t"
                     "ds_read_b128 %8, %12 offset:%19\n\tds_read_b128 %9, %12 offset:%20\n\ts_waitcnt lgkmcnt(0)"
                     : "=&v"(lo), "=&v"(hi), "=&v"(wh[0]), "=&v"(wl[0]), "=&v"(wh[1]), "=&v"(wl[1]), "=&v"(wh[2]), "=&v"(wl[2]),
                       "=&v"(wh[3]), "=&v"(wl[3])
                     : "v"(a0), "v"(a1), "v"(b), "n"(OFF), "n"(OFF + PL), "n"(OFF + 1024), "n"(OFF + PL + 1024),
                       "n"(OFF + 2048), "n"(OFF + PL + 2048), "n"(OFF + 3072), "n"(OFF + PL + 3072) : "memory");
}
// N consecutive 1-KiB LDS-DMA pieces (64 lanes x 16 bytes): src is this lane's address in the first piece, dst uniform
template <int N> __device__ __forceinline__ void gl_dma_pieces(const unsigned char* src, unsigned dst)
{
    gl_static_for<N>([&](auto PC) {
        constexpr int pc = decltype(PC)::value;
        __builtin_amdgcn_global_load_lds((gbl_void*)(src + pc * 1024), (lds_void*)(size_t)(dst + pc * 1024), 16, 0, 0);
    });
}

// One pipelined unit: the ds_reads of the NEXT unit's A / B fragments interleaved with the MFMAs of the current unit
// (al * wd, ah * wl, ah * wh per tile: the order of f3_mac3; wd lifted by the caller), closed by the lgkmcnt wait -- one asm block, so no
// register is visible to hipcc while it is in flight.  (`s_nop 1`: the operands come from VALU instructions right
// before the block -- 2 wait states to an MFMA read.)
template <int TN, int OFF, int PL>
__device__ __forceinline__ void gl_read_next_mfma(f32x4& nlo, f32x4& nhi, f16x8 (&nwh)[TN], f16x8 (&nwl)[TN],
                                                  f32x16 (&acc)[TN], const f16x8& al, const f16x8& ah,
                                                  const f16x8 (&wd)[TN], const f16x8 (&wl)[TN], const f16x8 (&wh)[TN],
                                                  unsigned a0, unsigned a1, unsigned b)
{
    static_assert(TN == 1 || TN == 2, "tile counts of the pipelined channel pairs");
    if constexpr (TN == 1)
        asm volatile("s_nop 1\n\t"
                     "ds_read_b128 %0, %10\n\tds_read_b128 %1, %11\n\t"
                     "v_mfma_f32_32x32x16_f16 %4, %5, %7, %4\n\t"
                     "ds_read_b128 %2, %12 offset:%13\n\tds_read_b128 %3, %12 offset:%14\n\t"
                     "v_mfma_f32_32x32x16_f16 %4, %6, %8, %4\n\t"
                     "v_mfma_f32_32x32x16_f16 %4, %6, %9, %4\n\t"
                     "s_waitcnt lgkmcnt(0)"
                     : "=&v"(nlo), "=&v"(nhi), "=&v"(nwh[0]), "=&v"(nwl[0]), "+v"(acc[0])
                     : "v"(al), "v"(ah), "v"(wd[0]), "v"(wl[0]), "v"(wh[0]), "v"(a0), "v"(a1), "v"(b), "n"(OFF), "n"(OFF + PL)
                     : "memory");
    else
        asm volatile("s_nop 1\n\t"
                     "ds_read_b128 %0, %16\n\tds_read_b128 %1, %17\n\t"
                     "v_mfma_f32_32x32x16_f16 %6, %8, %10, %6\n\t"
                     "v_mfma_f32_32x32x16_f16 %7, %8, %13, %7\n\t"
                     "ds_read_b128 %2, %18 offset:%19\n\tds_read_b128 %3, %18 offset:%20\n\t"
                     "v_mfma_f32_32x32x16_f16 %6, %9, %11, %6\n\t"
                     "v_mfma_f32_32x32x16_f16 %7, %9, %14, %7\n\t"
                     "ds_read_b128 %4, %18 offset:%21\n\tds_read_b128 %5, %18 offset:%22\n\t"
                     "v_mfma_f32_32x32x16_f16 %6, %9, %12, %6\n\t"
                     "v_mfma_f32_32x32x16_f16 %7, %9, %15, %7\n\t"
                     "s_waitcnt lgkmcnt(0)"
                     : "=&v"(nlo), "=&v"(nhi), "=&v"(nwh[0]), "=&v"(nwl[0]), "=&v"(nwh[1]), "=&v"(nwl[1]), "+v"(acc[0]), "+v"(acc[1])
                     : "v"(al), "v"(ah), "v"(wd[0]), "v"(wl[0]), "v"(wh[0]), "v"(wd[1]), "v"(wl[1]), "v"(wh[1]),
                       "v"(a0), "v"(a1), "v"(b), "n"(OFF), "n"(OFF + PL), "n"(OFF + 1024), "n"(OFF + PL + 1024)
                     : "memory");
}

// ---------------------------------------------------------------------------------------------- host side
// The argument checks of an f16x3 sparse entry point, in their one order; `name` is the name the messages carry (an
// _io / _tiles_io entry point checks what is its own under its own name, then shares the plain entry point's checks).
// sizes_ok / sizes_msg: what the structure asks of K (and Cin); ptrs: every pointer it reads is there; nbr_pitch: of a
// tiled table, or -1 (the plain rulebook: no pitch rule).  *run = false with AL3D_OK: no rows, nothing to launch --
// decided before the pointers are looked at.
static int sp_conv_check(const char* name, bool sizes_ok, const char* sizes_msg, int io, int n_out, bool ptrs,
                         const float* scale, int nbr_pitch, bool* run)
{
    *run = false;
    AL3D_REQUIRE(sizes_ok && n_out >= 0, "%s: %s", name, sizes_msg);
    AL3D_REQUIRE(io >= 0 && io < 8, "%s: bad io flags", name);
    if (n_out == 0) return AL3D_OK;
    AL3D_REQUIRE(ptrs, "%s: null pointer", name);
    AL3D_REQUIRE(scale, "%s: scale carries the weight exponent and is required", name);
    AL3D_REQUIRE(nbr_pitch == -1 || (nbr_pitch >= n_out && nbr_pitch % 256 == 0),
                 "%s: nbr_pitch must be al3d_sp_table_pitch(n_out)", name);
    *run = true;
    return AL3D_OK;
}

// Launches kernel(args...) -- the arguments converted to the kernel's parameter types -- and reports a launch error under
// `what`: a row of a file's dispatch table is `if (cin == .. && cout == ..) return sp_launch(..)`
template <class... KA, class... A>
static int sp_launch(const char* what, void (*kernel)(KA...), int64_t grid, int block, void* stream, A... args)
{
    hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3((unsigned)block), 0, (hipStream_t)stream, (KA)args...);
    AL3D_CHECK_LAUNCH(what);
    return AL3D_OK;
}
