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

// ---- textures (include/sge_amd_render_textures.h) ----

// a float every lane holds, as a scalar
__device__ __forceinline__ float uniformFloat(float v) { return __uint_as_float((unsigned)uniformInt((int)__float_as_uint(v))); }

// The pinned sampler: clamp-to-edge, level 0, bilinear, decode before filtering. Four plain loads of packed words; in the frame
// kernels every lane of the pixel's wavefront asks for the same uv, so the addresses are wave-uniform.
__device__ __forceinline__ void texDecode(uint32_t w, bool srgb, const float* table, float out[4]) {
    const uint32_t r = w & 255u, g = (w >> 8) & 255u, b = (w >> 16) & 255u, a = w >> 24;
    out[0] = srgb ? table[r] : (float)r / 255.0f;
    out[1] = srgb ? table[g] : (float)g / 255.0f;
    out[2] = srgb ? table[b] : (float)b / 255.0f;
    out[3] = (float)a / 255.0f;
}
__device__ __forceinline__ void texSample(const DevRenderTexture& t, const float* table, float u, float v, float out[4]) {
    const int W = t.width, H = t.height;
    const float x = fminf(fmaxf(u * (float)W - 0.5f, 0.0f), (float)(W - 1));
    const float y = fminf(fmaxf(v * (float)H - 0.5f, 0.0f), (float)(H - 1));
    const int x0 = (int)floorf(x), y0 = (int)floorf(y);
    const int x1 = min(x0 + 1, W - 1), y1 = min(y0 + 1, H - 1);
    const float fx = x - (float)x0, fy = y - (float)y0;
    const bool srgb = t.format == SGE_TEX_RGBA8_UNORM_SRGB;
    const uint32_t* r0 = t.texels + (size_t)y0 * W;
    const uint32_t* r1 = t.texels + (size_t)y1 * W;
    float t00[4], t10[4], t01[4], t11[4];
    texDecode(r0[x0], srgb, table, t00);
    texDecode(r0[x1], srgb, table, t10);
    texDecode(r1[x0], srgb, table, t01);
    texDecode(r1[x1], srgb, table, t11);
    for (int k = 0; k < 4; ++k) {
        const float top = t00[k] * (1.0f - fx) + t10[k] * fx;
        const float bot = t01[k] * (1.0f - fx) + t11[k] * fx;
        out[k] = top * (1.0f - fy) + bot * fy;
    }
}

// ---- specular IBL (include/sge_amd_render_ibl.h) ----

// the face selection of the header and the inverse of cubeDirection (IBLResources.swift:93-104)
struct CubeCoord { int face; float u, v; };
__device__ __forceinline__ CubeCoord cubeCoordOf(F3 d) {
    const float ax = fabsf(d.x), ay = fabsf(d.y), az = fabsf(d.z);
    if (ax >= ay && ax >= az) return d.x < 0.0f ? CubeCoord{1, d.z / ax, -d.y / ax} : CubeCoord{0, -d.z / ax, -d.y / ax};
    if (ay >= az) return d.y < 0.0f ? CubeCoord{3, d.x / ay, -d.z / ay} : CubeCoord{2, d.x / ay, d.z / ay};
    return d.z < 0.0f ? CubeCoord{5, -d.x / az, -d.y / az} : CubeCoord{4, d.x / az, -d.y / az};
}
// cubeDirection, not normalised
__device__ __forceinline__ F3 cubeDirectionOf(int face, float u, float v) {
    switch (face) {
    case 0: return F3{1.0f, -v, -u};
    case 1: return F3{-1.0f, -v, u};
    case 2: return F3{u, 1.0f, v};
    case 3: return F3{u, -1.0f, -v};
    case 4: return F3{u, -v, 1.0f};
    default: return F3{-u, -v, -1.0f};
    }
}
// One tap of a level whose faces are n x n: (i, j) in -1 .. n; a tap outside the face reads the texel that holds the direction of
// its centre. Every index that reaches the load is inside 0 .. n - 1 and face inside 0 .. 5, whatever the inputs were.
__device__ __forceinline__ F3 cubeTap(const uint16_t* level, int n, int face, int i, int j) {
    if (i < 0 || i >= n || j < 0 || j >= n) {
        const float uc = (2.0f * ((float)i + 0.5f)) / (float)n - 1.0f;
        const float vc = (2.0f * ((float)j + 0.5f)) / (float)n - 1.0f;
        const CubeCoord c = cubeCoordOf(cubeDirectionOf(face, uc, vc));
        face = c.face;
        i = min(max((int)floorf(((c.u + 1.0f) * 0.5f) * (float)n), 0), n - 1);
        j = min(max((int)floorf(((c.v + 1.0f) * 0.5f) * (float)n), 0), n - 1);
    }
    const uint2 w = *reinterpret_cast<const uint2*>(level + (((size_t)face * n + j) * n + i) * 4);
    const _Float16 r = __builtin_bit_cast(_Float16, (uint16_t)(w.x & 0xffffu));
    const _Float16 g = __builtin_bit_cast(_Float16, (uint16_t)(w.x >> 16));
    const _Float16 b = __builtin_bit_cast(_Float16, (uint16_t)(w.y & 0xffffu));
    return F3{(float)r, (float)g, (float)b};
}
__device__ __forceinline__ F3 cubeLevelSample(const RenderIBL& I, int l, const CubeCoord& c) {
    const int n = max(I.size >> l, 1);
    const uint16_t* level = I.env + (size_t)I.levelOff[l] * 4;
    const float x = fminf(fmaxf(((c.u + 1.0f) * 0.5f) * (float)n - 0.5f, -0.5f), (float)n - 0.5f);
    const float y = fminf(fmaxf(((c.v + 1.0f) * 0.5f) * (float)n - 0.5f, -0.5f), (float)n - 0.5f);
    const int x0 = (int)floorf(x), y0 = (int)floorf(y);
    const int x1 = x0 + 1, y1 = y0 + 1;
    const float fx = x - (float)x0, fy = y - (float)y0;
    const F3 t00 = cubeTap(level, n, c.face, x0, y0), t10 = cubeTap(level, n, c.face, x1, y0);
    const F3 t01 = cubeTap(level, n, c.face, x0, y1), t11 = cubeTap(level, n, c.face, x1, y1);
    const F3 top = t00 * (1.0f - fx) + t10 * fx;
    const F3 bot = t01 * (1.0f - fx) + t11 * fx;
    return top * (1.0f - fy) + bot * fy;
}
// envMap.sample(samp, d, level(lod)).xyz
__device__ __forceinline__ F3 envSample(const RenderIBL& I, F3 d, float lod) {
    const float mip = fminf(fmaxf(lod, 0.0f), (float)(I.mipCount - 1));
    const int l0 = (int)floorf(mip);
    const int l1 = min(l0 + 1, I.mipCount - 1);
    const float fl = mip - (float)l0;
    const CubeCoord c = cubeCoordOf(d);
    const F3 c0 = cubeLevelSample(I, l0, c), c1 = cubeLevelSample(I, l1, c);
    return c0 * (1.0f - fl) + c1 * fl;
}
// brdfLUT.sample(samp, (u, v)).xy: texSample's coordinates and filter over float texels
__device__ __forceinline__ void brdfLutSample(const RenderIBL& I, float u, float v, float out[2]) {
    const int W = I.lutW, H = I.lutH;
    const float x = fminf(fmaxf(u * (float)W - 0.5f, 0.0f), (float)(W - 1));
    const float y = fminf(fmaxf(v * (float)H - 0.5f, 0.0f), (float)(H - 1));
    const int x0 = (int)floorf(x), y0 = (int)floorf(y);
    const int x1 = min(x0 + 1, W - 1), y1 = min(y0 + 1, H - 1);
    const float fx = x - (float)x0, fy = y - (float)y0;
    const float2* r0 = reinterpret_cast<const float2*>(I.lut + (size_t)y0 * W * 4);
    const float2* r1 = reinterpret_cast<const float2*>(I.lut + (size_t)y1 * W * 4);
    const float2 t00 = r0[x0 * 2], t10 = r0[x1 * 2], t01 = r1[x0 * 2], t11 = r1[x1 * 2];
    const float topx = t00.x * (1.0f - fx) + t10.x * fx, botx = t01.x * (1.0f - fx) + t11.x * fx;
    const float topy = t00.y * (1.0f - fx) + t10.y * fx, boty = t01.y * (1.0f - fx) + t11.y * fx;
    out[0] = topx * (1.0f - fy) + botx * fy;
    out[1] = topy * (1.0f - fy) + boty * fy;
}
// eval_spec_ibl (RayTracing.metalinc:88-104). In the frame kernels every lane holds the same N, V and surface: R, the level and
// the table's coordinate are made scalar, so every tap is a wave-uniform load.
__device__ __forceinline__ F3 evalSpecIbl(const RenderIBL& I, F3 N, F3 V, float roughness, float metallic, F3 base) {
    const float NoV = uniformFloat(sat(dot(N, V)));
    const F3 In = -V;
    const F3 Rr = In - N * (2.0f * dot(N, In));
    const F3 Rd{uniformFloat(Rr.x), uniformFloat(Rr.y), uniformFloat(Rr.z)};
    const float rough = uniformFloat(roughness);
    const float mip = rough * fmaxf((float)(I.mipCount - 1), 0.0f);
    const F3 prefiltered = envSample(I, Rd, mip);
    float brdf[2];
    brdfLutSample(I, NoV, rough, brdf);
    const F3 F0 = F3{0.04f, 0.04f, 0.04f} + (base - F3{0.04f, 0.04f, 0.04f}) * metallic;
    return mul(prefiltered, F0 * brdf[0] + F3{brdf[1], brdf[1], brdf[1]});
}

// The hit record of sge_scene_intersect_* at a hit the scan reported: blasHitRecord over whichever half's streams hold the
// triangle, as the tail of sge_scene_trace_body.inc calls it. (u, v) are the barycentrics the walk left.
template <int STRIDE, class Crowd>
__device__ __forceinline__ void renderHitRecord(const SceneTrace& S, const Crowd& C, int inst, uint32_t prim, float u, float v, F3 wd, sge_blas_hit& H) {
    const BlasBest B{0.0f, u, v, prim, inst};
    H.uv[0] = 0.0f; H.uv[1] = 0.0f;
    if (inst >= SGE_SCENE_STATIC_BASE) {
        const int s = inst - SGE_SCENE_STATIC_BASE;
        const DevSceneMesh& m = S.meshes[S.meshOf[s]];
        blasHitRecord<3>(loadInstance(S.matrices, s), m.positions, m.normals, m.tangents, m.uvs, m.indices + (size_t)prim * 3, wd, B, H);
    } else {
        const BlasTrace& T = S.T;
        const CrowdStreams cs = C.streams(inst);
        const size_t vbase = cs.vbase;
        blasHitRecord<STRIDE>(loadInstance(T.instances, inst), reinterpret_cast<const float*>(T.positions) + vbase * STRIDE,
                              reinterpret_cast<const float*>(T.normals) + vbase * STRIDE, T.tangents + vbase * 4, cs.uvs,
                              cs.indices + (size_t)prim * 3, wd, B, H);
    }
}

// sample_alpha (RayTracing.metalinc:178-195): the occluder's alpha factor (clamped in the device table) times its texture's w
template <int STRIDE, class Crowd>
__device__ __forceinline__ float sampleAlpha(const SceneTrace& S, const RenderLaunch& R, const RenderTextures& X, const Crowd& C, int inst, uint32_t prim,
                                             float u, float v, F3 wd) {
    const int mat = materialOf(S, R, inst);
    float alpha = R.materials[mat].alpha;
    const int tex = X.bindings[mat].baseColor;
    if (tex >= 0) {
        sge_blas_hit H;
        renderHitRecord<STRIDE>(S, C, inst, prim, u, v, wd, H);
        float c[4];
        texSample(X.table[tex], X.srgb, H.uv[0], H.uv[1], c);
        alpha *= c[3];
    }
    return alpha;
}

// sample_material (:132-176) and the normal map (:283-316) at a surface: `m` is the sampled PBRSample in the fields of the material
// it starts from, N comes in as the face-forwarded geometric normal and leaves as the shading normal.
template <int STRIDE, class Crowd>
__device__ __forceinline__ void sampleSurface(const SceneTrace& S, const RenderLaunch& R, const RenderTextures& X, const Crowd& C, int inst, uint32_t prim,
                                              float u, float v, F3 wd, sge_render_material& m, F3& N) {
    const int mat = materialOf(S, R, inst);
    m = R.materials[mat];
    const sge_render_material_textures b = X.bindings[mat];
    if (b.baseColor < 0 && b.normal < 0 && b.metallicRoughness < 0 && b.emissive < 0 && b.occlusion < 0) return;
    sge_blas_hit H;
    renderHitRecord<STRIDE>(S, C, inst, prim, u, v, wd, H);
    const float tu = H.uv[0], tv = H.uv[1];
    float c[4];
    if (b.baseColor >= 0) {
        texSample(X.table[b.baseColor], X.srgb, tu, tv, c);
        m.baseColor[0] *= c[0]; m.baseColor[1] *= c[1]; m.baseColor[2] *= c[2];
        m.alpha *= c[3];
    }
    if (b.metallicRoughness >= 0) {
        texSample(X.table[b.metallicRoughness], X.srgb, tu, tv, c);
        m.roughness *= c[1];
        m.metallic *= c[2];
    }
    if (b.emissive >= 0) {
        texSample(X.table[b.emissive], X.srgb, tu, tv, c);
        m.emissive[0] *= c[0]; m.emissive[1] *= c[1]; m.emissive[2] *= c[2];
    }
    if (b.occlusion >= 0) {
        texSample(X.table[b.occlusion], X.srgb, tu, tv, c);
        m.occlusionStrength *= c[0];
    }
    if (b.normal >= 0) {
        texSample(X.table[b.normal], X.srgb, tu, tv, c);
        const float nx = c[0] * 2.0f - 1.0f, ny = c[1] * 2.0f - 1.0f;
        const float NoV = sat(dot(N, unit(-wd)));
        const float t = sat((NoV - 0.05f) / (0.5f - 0.05f));
        const float graze = (t * t) * (3.0f - 2.0f * t);
        const float ns = 4.0f + fmaxf(b.normalScale - 4.0f, 0.0f) * 0.25f;
        const float x = nx * (ns * graze), y = ny * (ns * graze);
        const float z = sqrtf(fmaxf(1.0f - (x * x + y * y), 0.0f));
        F3 n = unit((arr3(H.tangent) * x + arr3(H.bitangent) * y) + arr3(H.normal) * z);
        if (dot(n, wd) > 0.0f) n = -n;
        N = n;
    }
}

// what a pixel carries from query to query (see the kernel). TEX: the textured form keeps the sampled surfaces (sample_material's
// PBRSample, in the fields of sge_render_material) where the untextured one keeps the material indices.
template <bool TEX>
struct PixelStateT {
    F3 pHit, pN, pd, pColor; float pBias; int pMat;
    F3 sHit, sN, sd, direct, rd; float sBias, shadow; int sMat, li, sCount, pending;
    F3 accum; float accumAlpha; int layer, queries, phase;
    int aInst, aPrim, aFlags; float aDist, aShadow;
};
template <>
struct PixelStateT<true> {
    F3 pHit, pN, pd, pColor; float pBias; sge_render_material pSurf;
    F3 sHit, sN, sd, direct, rd; float sBias, shadow; sge_render_material sSurf; int li, sCount, pending;
    F3 accum; float accumAlpha; int layer, queries, phase;
    int aInst, aPrim, aFlags; float aDist, aShadow;
};
// the surface being shaded / the layer's surface once shaded
template <bool TEX>
__device__ __forceinline__ const sge_render_material& surfaceS(const PixelStateT<TEX>& ps, const RenderLaunch& R) {
    if constexpr (TEX) return ps.sSurf; else return R.materials[ps.sMat];
}
template <bool TEX>
__device__ __forceinline__ const sge_render_material& surfaceP(const PixelStateT<TEX>& ps, const RenderLaunch& R) {
    if constexpr (TEX) return ps.pSurf; else return R.materials[ps.pMat];
}

} // namespace


} // namespace sge
