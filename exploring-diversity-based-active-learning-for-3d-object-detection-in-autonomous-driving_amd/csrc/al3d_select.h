// Top-K selection of the detection heads, in one place (DESIGN.md "One selection header"): the sigmoid score, the
// workgroup scan, the sort word (al3d_sort_key.h), the one-workgroup bitonic sort and the radix threshold with its
// collect step.  The tie rule of every user: higher score first, equal scores by lower flat index.
// THREADS is the workgroup size, a multiple of 64 up to 1024; every thread of the workgroup makes every blk_* call.
#pragma once
#include "al3d_sort_key.h"

__device__ __forceinline__ float al3d_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

// LDS scratch of the blk_* functions below
template <int THREADS>
struct SelScratch {
    unsigned hist[256];
    unsigned prefix, need, count;
    int wave[THREADS / 64];
};

// exclusive sum of v over the workgroup in thread order; total = the sum of all.  s_wave: THREADS / 64 words of LDS
template <int THREADS>
__device__ __forceinline__ int blk_exclusive_scan(int v, int* s_wave, int& total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int x = v;                                          // inclusive scan inside the wave
    for (int off = 1; off < 64; off <<= 1) {
        const int y = __shfl_up(x, off);
        if (lane >= off) x += y;
    }
    if (lane == 63) s_wave[wave] = x;
    __syncthreads();
    if (wave == 0) {
        int w = lane < THREADS / 64 ? s_wave[lane] : 0;
        for (int off = 1; off < THREADS / 64; off <<= 1) {
            const int y = __shfl_up(w, off);
            if (lane >= off) w += y;
        }
        if (lane < THREADS / 64) s_wave[lane] = w;      // inclusive wave totals
    }
    __syncthreads();
    const int base = wave > 0 ? s_wave[wave - 1] : 0;
    total = s_wave[THREADS / 64 - 1];
    __syncthreads();
    return base + x - v;
}

// bitonic sort of w[0..N), descending; N a power of two (int or int64_t), w in LDS or global memory, written before a
// barrier.  A thread owns the compare-exchange (i, i | stride); distinct words give one result whatever the network.
template <int THREADS, typename I>
__device__ __forceinline__ void blk_sort_desc_u64(unsigned long long* w, I N)
{
    for (I size = 2; size <= N; size <<= 1)
        for (I stride = size >> 1; stride > 0; stride >>= 1) {
            for (I t = threadIdx.x; t < N / 2; t += THREADS) {
                const I i = ((t & ~(stride - 1)) << 1) | (t & (stride - 1)), j = i | stride;
                const unsigned long long x = w[i], y = w[j];
                if ((i & size) == 0 ? x < y : x > y) { w[i] = y; w[j] = x; }
            }
            __syncthreads();
        }
}

// T = the K-th largest of keys[0..N), N >= K >= 1; need = how many of the keys equal to T belong to the K largest.
// Four-pass radix select, most significant byte first, over a 256-bin LDS histogram.
template <int THREADS>
__device__ __forceinline__ void blk_radix_threshold(const unsigned* __restrict__ keys, int N, unsigned K, SelScratch<THREADS>& s,
                                                    unsigned& T, unsigned& need)
{
    const unsigned tid = threadIdx.x, lane = tid & 63u;
    unsigned prefix = 0u;
    need = K;
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        if (tid < 256) s.hist[tid] = 0u;
        __syncthreads();
        const unsigned hi_mask = pass == 0 ? 0u : 0xffffffffu << (shift + 8);
        for (unsigned i0 = 0; i0 < (unsigned)N; i0 += THREADS) {
            const unsigned i = i0 + tid;
            int bin = -1;
            if (i < (unsigned)N) {
                const unsigned v = keys[i];
                if ((v & hi_mask) == prefix) bin = (int)((v >> shift) & 255u);
            }
            // background scores share their leading byte: one aggregated atomic for the first lane's bin, plain LDS
            // atomics for the rest
            const unsigned long long pending = __ballot(bin >= 0);
            if (pending) {
                const int leader = (int)__builtin_ctzll(pending);
                const int lb = __shfl(bin, leader);
                const unsigned long long same = __ballot(bin == lb);
                if ((int)lane == leader) atomicAdd(&s.hist[lb], (unsigned)__popcll(same));
                if (bin >= 0 && bin != lb) atomicAdd(&s.hist[bin], 1u);
            }
        }
        __syncthreads();
        if (tid == 0) {
            unsigned acc = 0u;
            int d = 255;
            for (; d > 0; --d) {
                if (acc + s.hist[d] >= need) break;
                acc += s.hist[d];
            }
            s.prefix = prefix | ((unsigned)d << shift);
            s.need = need - acc;
        }
        __syncthreads();
        prefix = s.prefix;
        need = s.need;
        __syncthreads();
    }
    T = prefix;
}

// dst[slot] = sel_word(key, index_base + i) for every key above T and for the first `need` keys equal to T in ascending
// i; slots in no order (the caller sorts), writes past `cap` dropped.  A thread owns a contiguous chunk of indices, so
// the scan of the per-thread tie counts ranks the ties by index.  Ends on a barrier.
template <int THREADS>
__device__ __forceinline__ void blk_collect_topk(const unsigned* __restrict__ keys, int N, unsigned T, unsigned need,
                                                 unsigned index_base, unsigned long long* dst, unsigned cap, SelScratch<THREADS>& s)
{
    if (threadIdx.x == 0) s.count = 0u;
    const unsigned n = (unsigned)N, chunk = (n + THREADS - 1) / THREADS;
    const unsigned i0 = threadIdx.x * chunk < n ? threadIdx.x * chunk : n, i1 = i0 + chunk < n ? i0 + chunk : n;
    int neq = 0;
    for (unsigned i = i0; i < i1; ++i) neq += keys[i] == T;
    int tot_eq;
    int peq = blk_exclusive_scan<THREADS>(neq, s.wave, tot_eq);          // barriers inside: s.count is visible
    for (unsigned i = i0; i < i1; ++i) {
        const unsigned v = keys[i];
        bool take = v > T;
        if (v == T) { take = peq < (int)need; ++peq; }
        if (take) {
            const unsigned slot = atomicAdd(&s.count, 1u);
            if (slot < cap) dst[slot] = sel_word(v, index_base + i);
        }
    }
    __syncthreads();
}
