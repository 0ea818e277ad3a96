// The 64-bit sort word of every top-K selection (al3d_select.h) and the key of al3d_argsort_desc_f32, in one place for
// the kernels and for the test suite's CPU check of the formula: plain C, no device intrinsics.
//
// word = (order-preserving 32 bits) << 32 | ~index; a larger word sorts first: bits descending, equal bits by ascending index.
#pragma once

#ifdef __HIPCC__
#define AL3D_SORT_KEY_FN __host__ __device__ __forceinline__
#else
#define AL3D_SORT_KEY_FN static inline
#endif

AL3D_SORT_KEY_FN unsigned long long sel_word(unsigned bits, unsigned index) { return ((unsigned long long)bits << 32) | (unsigned)~index; }
AL3D_SORT_KEY_FN unsigned sel_word_bits(unsigned long long w) { return (unsigned)(w >> 32); }
AL3D_SORT_KEY_FN unsigned sel_word_index(unsigned long long w) { return ~(unsigned)w; }

// torch.argsort(-x, stable=True): descending, NaN last, equal values by ascending index.
AL3D_SORT_KEY_FN unsigned long long al3d_sort_key(float v, unsigned idx)
{
    unsigned u;
    if (v != v) u = 0u;                                    // NaN (either sign): smallest key -> last
    else {
        __builtin_memcpy(&u, &v, sizeof(u));
        if (u == 0x80000000u) u = 0u;                       // -0.0 == +0.0: one key, index decides
        u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);     // total order, larger float -> larger key
    }
    return sel_word(u, idx);
}
