// Device-side body of the shaded frame (include/sge_amd_render.h), shared by render_frame_kernel (sge_render.hip) and its form
// for a crowd with mesh variants (sge_scene_variants.hip): the shading functions of raytraceKernel as the header pins them, and
// the pixel's state machine around one closest-hit scan per half of the scene. See sge_render.hip for the design.
#pragma once
#include "sge_ray_scene_dev.hpp"

namespace sge {

namespace {

// the header's normalize: v / sqrt(dot(v, v)) (sge_math.hpp's multiplies by the reciprocal; the hit record's normal keeps that)
__device__ __forceinline__ F3 unit(F3 v) { return v / sqrtf(dot(v, v)); }
__device__ __forceinline__ F3 mul(F3 a, F3 b) { return F3{a.x * b.x, a.y * b.y, a.z * b.z}; }
__device__ __forceinline__ float sat(float v) { return fminf(fmaxf(v, 0.0f), 1.0f); }
__device__ __forceinline__ F3 mix3(F3 a, F3 b, F3 t) { return a + mul(b - a, t); }
__device__ __forceinline__ F3 arr3(const float* p) { return F3{p[0], p[1], p[2]}; }

// RayTracing.metalinc:21-23
__device__ __forceinline__ F3 fresnelSchlick(float cosTheta, F3 F0) {
    const float p = powf(sat(1.0f - cosTheta), 5.0f);
    return F0 + (F3{1.0f, 1.0f, 1.0f} - F0) * p;
}
// :31-36
__device__ __forceinline__ float ggxG1(float NoV, float a) {
    const float a2 = a * a;
    const float denom = NoV + sqrtf(a2 + ((1.0f - a2) * NoV) * NoV);
    return (2.0f * NoV) / fmaxf(denom, 1e-4f);
}
// :42-59
__device__ __forceinline__ F3 evalBrdf(F3 N, F3 V, F3 L, F3 base, float metallic, float roughness) {
    const float NoL = sat(dot(N, L)), NoV = sat(dot(N, V));
    if (NoL <= 0.0f || NoV <= 0.0f) return F3{0, 0, 0};
    const F3 H = unit(V + L);
    const float NoH = sat(dot(N, H)), VoH = sat(dot(V, H));
    const float alpha = roughness * roughness;
    const F3 diff = (base * (1.0f - metallic)) * (1.0f / 3.14159265f);
    const float a2 = alpha * alpha;
    const float dd = (NoH * NoH) * (a2 - 1.0f) + 1.0f;
    const float D = a2 / ((3.14159265f * dd) * dd);
    const float G = ggxG1(NoV, alpha) * ggxG1(NoL, alpha);
    const F3 F0 = F3{0.04f, 0.04f, 0.04f} + (base - F3{0.04f, 0.04f, 0.04f}) * metallic;
    const F3 F = fresnelSchlick(VoH, F0);
    const F3 spec = (F * (D * G)) / fmaxf((4.0f * NoV) * NoL, 1e-4f);
    return diff + spec;
}
// :65-86
__device__ __forceinline__ F3 evalEnvSH(F3 n, const sge_render_frame& F) {
    const float x = n.x, y = n.y, z = n.z;
    const float c0 = 0.282095f, c1 = 0.488603f, c2 = 1.092548f, c3 = 0.315392f, c4 = 0.546274f;
    F3 r = arr3(F.envSH[0]) * c0;
    r = r + arr3(F.envSH[1]) * (c1 * y);
    r = r + arr3(F.envSH[2]) * (c1 * z);
    r = r + arr3(F.envSH[3]) * (c1 * x);
    r = r + arr3(F.envSH[4]) * ((c2 * x) * y);
    r = r + arr3(F.envSH[5]) * ((c2 * y) * z);
    r = r + arr3(F.envSH[6]) * (c3 * ((3.0f * z) * z - 1.0f));
    r = r + arr3(F.envSH[7]) * ((c2 * x) * z);
    r = r + arr3(F.envSH[8]) * (c4 * (x * x - y * y));
    return r;
}
// :15-19
__device__ __forceinline__ float fractf(float x) { return x - floorf(x); }
__device__ __forceinline__ float hash12(float px, float py) {
    F3 p3{fractf(px * 0.1031f), fractf(py * 0.1031f), fractf(px * 0.1031f)};
    const float d = dot(p3, F3{p3.y + 33.33f, p3.z + 33.33f, p3.x + 33.33f});
    p3 = F3{p3.x + d, p3.y + d, p3.z + d};
    return fractf((p3.x + p3.y) * p3.z);
}

__device__ __forceinline__ int materialOf(const SceneTrace& S, const RenderLaunch& R, int inst) {
    if (inst >= SGE_SCENE_STATIC_BASE) return R.staticMaterial ? R.staticMaterial[inst - SGE_SCENE_STATIC_BASE] : 0;
    return R.crowdMaterial ? R.crowdMaterial[inst] : 0;
}

// The face-forwarded geometric normal of the hit triangle: blasFaceNormal (sge_blas_trace_dev.hpp), which blasHitRecord fills
// geomNormal with for the same hit; here over whichever half's streams hold the triangle.
template <int STRIDE, class Crowd>
__device__ __forceinline__ F3 hitNormal(const SceneTrace& S, const Crowd& C, int inst, uint32_t prim, F3 wd) {
    const float* P; const uint32_t* ix; const float* Mf; int stride;
    if (inst >= SGE_SCENE_STATIC_BASE) {
        const int s = inst - SGE_SCENE_STATIC_BASE;
        const DevSceneMesh& m = S.meshes[S.meshOf[s]];
        P = m.positions; ix = m.indices + (size_t)prim * 3; Mf = S.matrices + (size_t)s * 16; stride = 3;
    } else {
        const BlasTrace& T = S.T;
        const CrowdStreams cs = C.streams(inst);
        P = reinterpret_cast<const float*>(T.positions) + cs.vbase * STRIDE;
        ix = cs.indices + (size_t)prim * 3; Mf = T.instances + (size_t)inst * 16; stride = STRIDE;
    }
    const Aff M{F3{Mf[0], Mf[1], Mf[2]}, F3{Mf[4], Mf[5], Mf[6]}, F3{Mf[8], Mf[9], Mf[10]}, F3{Mf[12], Mf[13], Mf[14]}};
    const float* a = P + (size_t)ix[0] * stride; const float* b = P + (size_t)ix[1] * stride; const float* c = P + (size_t)ix[2] * stride;
    return blasFaceNormal(M, arr3(a), arr3(b), arr3(c), wd);
}

// what a pixel carries from query to query (see the kernel)
struct PixelState {
    F3 pHit, pN, pd, pColor; float pBias; int pMat;
    F3 sHit, sN, sd, direct, rd; float sBias, shadow; int sMat, li, sCount, pending;
    F3 accum; float accumAlpha; int layer, queries, phase;
    int aInst, aPrim, aFlags; float aDist, aShadow;
};

} // namespace


} // namespace sge
