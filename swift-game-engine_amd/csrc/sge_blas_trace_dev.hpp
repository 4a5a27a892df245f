// Device-side pieces of the closest-hit query shared by blas_intersect_kernel / blas_world_boxes_kernel (sge_blas.hip: one
// topology for the whole crowd) and their ragged forms (sge_blas_variants.hip: one topology per mesh variant): the ray-triangle
// test, the instance transform and the widened slab test. A header of its own, not sge_blas_dev.hpp: that one is also included
// by sge_skin.hip, which has helpers of the same names.
#pragma once
#include "sge_internal.hpp"

namespace sge {

// Moller-Trumbore as the engine's own rayTriangle (CollisionQuery.swift:1575-1601), also returning the barycentrics
__device__ __forceinline__ bool rayTriangleUV(F3 origin, F3 direction, F3 v0, F3 v1, F3 v2, float eps, float& tOut, float& uOut, float& vOut) {
    F3 e1 = v1 - v0, e2 = v2 - v0;
    F3 pvec = cross(direction, e2);
    float det = dot(e1, pvec);
    if (fabsf(det) < eps) return false;
    float invDet = 1.0f / det;
    F3 tvec = origin - v0;
    float u = dot(tvec, pvec) * invDet;
    if (u < 0 || u > 1) return false;
    F3 qvec = cross(tvec, e1);
    float v = dot(direction, qvec) * invDet;
    if (v < 0 || (u + v) > 1) return false;
    float t = dot(e2, qvec) * invDet;
    if (!(t >= 0)) return false;
    tOut = t + 0.0f; // -0 -> +0
    uOut = u;
    vOut = v;
    return true;
}

struct Inv3 { F3 r0, r1, r2; float ok; }; // rows of the inverse of the 3x3 part
__device__ __forceinline__ Inv3 inverse3(const Aff& m) {
    const F3 a = m.c0, b = m.c1, c = m.c2;
    const F3 bc = cross(b, c), ca = cross(c, a), ab = cross(a, b);
    const float det = dot(a, bc);
    const float r = 1.0f / det;
    return Inv3{bc * r, ca * r, ab * r, det};
}
__device__ __forceinline__ F3 mul3(const Inv3& m, F3 v) { return F3{dot(m.r0, v), dot(m.r1, v), dot(m.r2, v)}; }

template <int STRIDE>
__device__ __forceinline__ F3 loadP(const float* base, uint32_t i) { const float* p = base + (size_t)i * STRIDE; return F3{p[0], p[1], p[2]}; }

constexpr int kBlasStack = kBlasTraversalStackCap;

__device__ __forceinline__ Aff loadInstance(const float* instances, int inst) {
    const float* Mf = instances + (size_t)inst * 16;
    return Aff{F3{Mf[0], Mf[1], Mf[2]}, F3{Mf[4], Mf[5], Mf[6]}, F3{Mf[8], Mf[9], Mf[10]}, F3{Mf[12], Mf[13], Mf[14]}};
}

// widened slab test (CollisionQuery.swift:1603-1630 form): a box is only skipped when it is clearly off the ray or clearly
// behind the best hit
__device__ __forceinline__ bool slabPass(const float* bx, F3 o, F3 inv, float tMin, float bestT) {
    float t0 = (bx[0] - o.x) * inv.x, t1 = (bx[3] - o.x) * inv.x;
    float lo = fminf(t0, t1), hi = fmaxf(t0, t1);
    t0 = (bx[1] - o.y) * inv.y; t1 = (bx[4] - o.y) * inv.y;
    lo = fmaxf(lo, fminf(t0, t1)); hi = fminf(hi, fmaxf(t0, t1));
    t0 = (bx[2] - o.z) * inv.z; t1 = (bx[5] - o.z) * inv.z;
    lo = fmaxf(lo, fminf(t0, t1)); hi = fminf(hi, fmaxf(t0, t1));
    const float slack = 1e-3f * fmaxf(fabsf(lo), fabsf(hi)) + 1e-4f;
    return (lo - slack <= hi + slack) && (hi + slack >= tMin) && (lo - slack <= bestT);
}
__device__ __forceinline__ F3 invDir(F3 d) {
    return F3{d.x != 0 ? 1.0f / d.x : kFloatMax, d.y != 0 ? 1.0f / d.y : kFloatMax, d.z != 0 ? 1.0f / d.z : kFloatMax};
}

} // namespace sge
