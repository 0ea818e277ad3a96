// Sort key of al3d_argsort_desc_f32, in one place for the kernel and for the test suite's CPU
// check of the formula: plain C, no device intrinsics.
//
// torch.argsort(-x, stable=True): descending, NaN last, equal values by ascending index.
// key = (order-preserving bits of x) << 32 | ~index; a larger key sorts first.
#pragma once

#ifdef __HIPCC__
#define AL3D_SORT_KEY_FN __host__ __device__ __forceinline__
#else
#define AL3D_SORT_KEY_FN static inline
#endif

AL3D_SORT_KEY_FN unsigned long long al3d_sort_key(float v, unsigned idx)
{
    unsigned u;
    if (v != v) u = 0u;                                    // NaN (either sign): smallest key -> last
    else {
        __builtin_memcpy(&u, &v, sizeof(u));
        if (u == 0x80000000u) u = 0u;                       // -0.0 == +0.0: one key, index decides
        u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);     // total order, larger float -> larger key
    }
    return ((unsigned long long)u << 32) | (unsigned)(0xffffffffu - idx);
}
