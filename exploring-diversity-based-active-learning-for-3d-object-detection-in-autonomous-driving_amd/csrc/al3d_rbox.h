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
    // orientation of the clip polygon
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
    float area = 0.f;
    for (int k = 0; k < n; ++k) { const int k2 = k + 1 == n ? 0 : k + 1; area += px[k] * py[k2] - px[k2] * py[k]; }
    return 0.5f * fabsf(area);
}

__device__ __forceinline__ float quad_area(const float* x, const float* y)
{
    float a = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) { const int k2 = (k + 1) & 3; a += x[k] * y[k2] - x[k2] * y[k]; }
    return 0.5f * fabsf(a);
}
