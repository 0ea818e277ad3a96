// Rotated-rectangle geometry shared by the anchor head's NMS (head_nms.hip) and the CenterPoint head's (center_head.hip):
// corners of a BEV box, area of a quadrilateral, intersection area of two convex quadrilaterals.  f32, no contraction.
#pragma once
#include <hip/hip_runtime.h>

// corners of (x, y, w, l, r): unit square (0,0),(0,1),(1,1),(1,0) minus 0.5, scaled by (w,l),
// rotated by [[cos,-sin],[sin,cos]] applied as row-vector @ R^T ... the reference's
// rotation_2d: einsum("aij,jka->aik", points, [[c,-s],[s,c]])  => x' = x*c + y*s, y' = -x*s + y*c
__device__ __forceinline__ void box_corners(float x, float y, float w, float l, float r, float* cx,
                                            float* cy)
{
    const float c = cosf(r), s = sinf(r);
    const float ux[4] = {-0.5f, -0.5f, 0.5f, 0.5f}, uy[4] = {-0.5f, 0.5f, 0.5f, -0.5f};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float px = ux[k] * w, py = uy[k] * l;
        cx[k] = px * c + py * s + x;
        cy[k] = -px * s + py * c + y;
    }
}

// area of the intersection of two convex quadrilaterals (Sutherland-Hodgman clip + shoelace)
__device__ float quad_intersection_area(const float* ax, const float* ay, const float* bx, const float* by)
{
    float px[10], py[10], qx[10], qy[10];
    int n = 4;
#pragma unroll
    for (int k = 0; k < 4; ++k) { px[k] = ax[k]; py[k] = ay[k]; }
    // orientation of the clip polygon: only the SIGN of this shoelace is used, so it stays on absolute coordinates -- twice
    // the area of the smallest real footprint is 0.32 m^2 against ~1e-3 m^2 of rounding at 54 m; a box too small for that
    // has no area worth clipping
    float barea = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) { const int k2 = (k + 1) & 3; barea += bx[k] * by[k2] - bx[k2] * by[k]; }
    const float sgn = barea >= 0.f ? 1.f : -1.f;
    for (int e = 0; e < 4 && n > 0; ++e) {
        const int e2 = (e + 1) & 3;
        const float ex = bx[e2] - bx[e], ey = by[e2] - by[e];
        int m = 0;
        for (int k = 0; k < n; ++k) {
            const int k2 = k + 1 == n ? 0 : k + 1;
            const float d1 = sgn * (ex * (py[k] - by[e]) - ey * (px[k] - bx[e]));
            const float d2 = sgn * (ex * (py[k2] - by[e]) - ey * (px[k2] - bx[e]));
            if (d1 >= 0.f) { qx[m] = px[k]; qy[m] = py[k]; ++m; }
            if ((d1 >= 0.f) != (d2 >= 0.f)) {
                const float tt = d1 / (d1 - d2);
                qx[m] = px[k] + tt * (px[k2] - px[k]);
                qy[m] = py[k] + tt * (py[k2] - py[k]);
                ++m;
            }
        }
        n = m;
        for (int k = 0; k < n; ++k) { px[k] = qx[k]; py[k] = qy[k]; }
    }
    if (n < 3) return 0.f;
    // shoelace about the first vertex: see quad_area
    float area = 0.f;
    for (int k = 1; k + 1 < n; ++k) area += (px[k] - px[0]) * (py[k + 1] - py[0]) - (px[k + 1] - px[0]) * (py[k] - py[0]);
    return 0.5f * fabsf(area);
}

// Shoelace about the quadrilateral's first vertex, not about the frame's origin: the products are then of the size of the
// box, not of its distance from the origin.  54 m out a product of absolute coordinates is ~2900 with an ulp of 2.4e-4 m^2,
// 0.15 % of a traffic cone's footprint: measured IoU error 3e-3 there against 1e-5 in this form (tests/anchorhead_cases.py).
__device__ __forceinline__ float quad_area(const float* x, const float* y)
{
    float a = 0.f;
#pragma unroll
    for (int k = 1; k < 3; ++k) a += (x[k] - x[0]) * (y[k + 1] - y[0]) - (x[k + 1] - x[0]) * (y[k] - y[0]);
    return 0.5f * fabsf(a);
}
