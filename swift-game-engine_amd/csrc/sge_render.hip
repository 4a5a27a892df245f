// The shaded frame for gfx950 (include/sge_amd_render.h): raytraceKernel (RayTracing.metalinc:197-730) over the ray scene, with
// frame.textureCount == 0 and without specular IBL.
//
// render_frame_kernel — one wavefront per pixel, plain launch, the LDS traversal stack and the closest-hit walk of
// scene_trace_kernel (sge_ray_scene_dev.hpp, sge_blas_trace_dev.hpp). The reference inlines its intersector at seven call sites
// (the layer's ray, its shadow walk, the mirror ray and its shadow walk, the refraction ray and its shadow walks). Here the pixel
// is a small state machine around ONE closest-hit scan per half of the scene: every pass of the loop issues the pending query
// (qo, qd, qmin, qmax), then advances the state — `mode` says whether the query was a surface ray or a step of a shadow walk,
// `phase` which surface is being shaded (0: the layer's own, 1: the mirror bounce, 2: the refraction bounce) — until the next
// query is set up or the pixel is done. The sections behind the scan run at most once per pass and each exists once in the
// code: the shadow step, the surface set-up, the light loop (eval_brdf), the surface's colour, the end of a bounce (the two
// mixes), the refraction set-up, the compositing. Shading is wave-uniform: the winner of the scan is made scalar
// (readfirstlane), every lane computes the same colour, lane 0 writes it.
//
// Every loop is bounded by a count read before it starts: a pixel issues at most 3 * (1 + 4 + 1 + 4 + 1 + 4 * lights) queries
// (three layers; the layer's ray and light 0's walk, the same for the mirror bounce, the refraction ray and a walk per light),
// the light loop runs at most lights + 1 times per pass.
//
// Built with -ffp-contract=off: what decides a ray is the float32 expression the header pins, as written.
#include "sge_ray_scene_dev.hpp"

namespace sge {

namespace {

// the header's normalize: v / sqrt(dot(v, v)) (sge_math.hpp's multiplies by the reciprocal; the hit record's normal keeps that)
__device__ __forceinline__ F3 unit(F3 v) { return v / sqrtf(dot(v, v)); }
__device__ __forceinline__ F3 mul(F3 a, F3 b) { return F3{a.x * b.x, a.y * b.y, a.z * b.z}; }
__device__ __forceinline__ float sat(float v) { return fminf(fmaxf(v, 0.0f), 1.0f); }
__device__ __forceinline__ F3 mix3(F3 a, F3 b, F3 t) { return a + mul(b - a, t); }
__device__ __forceinline__ F3 arr3(const float* p) { return F3{p[0], p[1], p[2]}; }
__device__ __forceinline__ int uniformInt(int v) { return __builtin_amdgcn_readfirstlane(v); }

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
template <int STRIDE>
__device__ __forceinline__ F3 hitNormal(const SceneTrace& S, int inst, uint32_t prim, F3 wd) {
    const float* P; const uint32_t* ix; const float* Mf; int stride;
    if (inst >= SGE_SCENE_STATIC_BASE) {
        const int s = inst - SGE_SCENE_STATIC_BASE;
        const DevSceneMesh& m = S.meshes[S.meshOf[s]];
        P = m.positions; ix = m.indices + (size_t)prim * 3; Mf = S.matrices + (size_t)s * 16; stride = 3;
    } else {
        const BlasTrace& T = S.T;
        P = reinterpret_cast<const float*>(T.positions) + (size_t)inst * T.blas.vertexCount * STRIDE;
        ix = T.indices + (size_t)prim * 3; Mf = T.instances + (size_t)inst * 16; stride = STRIDE;
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

// STRIDE: floats per vertex of the crowd's skinned positions
template <int STRIDE>
__global__ __launch_bounds__(kWave) void render_frame_kernel(const RenderArgs* A) {
    __shared__ int stack[kBlasStack];
    const int lane = threadIdx.x;
    // (the two records are read where they are used, from device memory: as kernel arguments they were held in scalar registers
    // across the whole loop, more of them than there are)
    const SceneTrace& S = A->S;
    const RenderLaunch& R = A->R;
    const sge_render_frame& F = R.frame;
    const BlasTrace& T = S.T;
    const int W = F.width, H = F.height;
    const int pixel = blockIdx.x;
    if (pixel >= W * H) return;
    const int gx = pixel % W, gy = pixel / W;
    const F3 cam = arr3(F.cameraPosition);

    // the camera ray, RayTracing.metalinc:225-235
    F3 dir;
    {
        const float px = ((float)gx + 0.5f) / (float)W, py = ((float)gy + 0.5f) / (float)H;
        const float nx = px * 2.0f - 1.0f, ny = (1.0f - py) * 2.0f - 1.0f;
        const float* m = F.invViewProj;
        float w4[4];
        for (int k = 0; k < 4; ++k) w4[k] = ((m[k] * nx + m[4 + k] * ny) + m[8 + k] * 1.0f) + m[12 + k] * 1.0f;
        dir = unit(F3{w4[0] / w4[3], w4[1] / w4[3], w4[2] / w4[3]} - cam);
    }

    const int nLights = F.dirLightCount;
    const int maxQueries = 3 * (11 + 4 * nLights);
    const F3 bg{0.02f, 0.02f, 0.03f};

    // the pending query
    F3 qo = cam, qd = dir;
    float qmin = 0.001f, qmax = 1e6f;
    int mode = 0;
    // Everything but the pending query lives in LDS while the scan runs (every lane holds the same values and stores the same
    // words; the scan's barriers keep the compiler from carrying them in registers across it): the registers belong to the walk.
    __shared__ PixelState ps;
    // the layer's surface once shaded, kept while a bounce is shaded
    F3 &pHit = ps.pHit, &pN = ps.pN, &pd = ps.pd, &pColor = ps.pColor;
    float& pBias = ps.pBias;
    int& pMat = ps.pMat;
    // the surface being shaded
    F3 &sHit = ps.sHit, &sN = ps.sN, &sd = ps.sd, &direct = ps.direct, &rd = ps.rd;
    float &sBias = ps.sBias, &shadow = ps.shadow;
    int &sMat = ps.sMat, &li = ps.li, &sCount = ps.sCount, &pending = ps.pending;
    // the pixel
    F3& accum = ps.accum;
    float& accumAlpha = ps.accumAlpha;
    int &layer = ps.layer, &queries = ps.queries, &phase = ps.phase;
    int &aInst = ps.aInst, &aPrim = ps.aPrim, &aFlags = ps.aFlags;
    float &aDist = ps.aDist, &aShadow = ps.aShadow;
    pHit = F3{0, 0, 0}; pN = F3{0, 0, 1}; pd = dir; pColor = F3{0, 0, 0}; pBias = 0; pMat = 0;
    sHit = F3{0, 0, 0}; sN = F3{0, 0, 1}; sd = dir; direct = F3{0, 0, 0}; rd = dir; sBias = 0; shadow = 1.0f;
    sMat = 0; li = 0; sCount = 0; pending = 0;
    accum = F3{0, 0, 0}; accumAlpha = 0; layer = 0; queries = 0; phase = 0;
    aInst = -1; aPrim = -1; aFlags = 0; aDist = 0; aShadow = 1.0f;

    BlasBest best{qmax, 0, 0, 0u, -1};
    auto visitStatic = [&](int s) {
        blasTraverseClosest<3, true>(stack, lane, sceneTree(S.meshes[S.meshOf[s]]), loadInstance(S.matrices, s), qo, qd, fmaxf(qmin, 0.0f), qmax,
                                     SGE_SCENE_STATIC_BASE + s, best);
        return false;
    };
    auto visitCharacter = [&](int inst) {
        blasTraverseClosest<STRIDE, true>(stack, lane, crowdTree<STRIDE>(T, inst), loadInstance(T.instances, inst), qo, qd, fmaxf(qmin, 0.0f), qmax, inst, best);
        return false;
    };

    bool done = false;
    for (int q = 0; q < maxQueries && !done; ++q) {
        // ---- the query: scene_trace_kernel's two halves for a ray that names no instance ----
        best = BlasBest{qmax, 0, 0, 0u, -1};
        {
            const float tMin = smax(qmin, 0.0f);
            const F3 inv = invDir(qd);
            if (S.statics > 0)
                sceneScan(S.boxes, S.boxes + (size_t)S.statics * 6, nullptr, nullptr, S.statics, -1, lane, qo, inv, tMin, best.t, visitStatic);
            if (S.crowd) {
                const int* order = T.instOrder;
                sceneScan(T.worldBoxes, order ? T.groupBoxes : T.worldBoxes + (size_t)T.chars * 6, order ? T.superBoxes : nullptr, order, T.chars, -1, lane,
                          qo, inv, tMin, best.t, visitCharacter);
            }
        }
        ++queries;
        const int hInst = uniformInt(best.inst);
        const uint32_t hPrim = (uint32_t)uniformInt((int)best.prim);
        const float hT = __uint_as_float((unsigned)uniformInt((int)__float_as_uint(best.t)));
        const bool hit = hInst >= 0;

        bool runLights = false, surfaceDone = false, bounceDone = false, checkRefraction = false, composite = false;
        F3 bAccum{0, 0, 0};
        float bAlpha = 0;

        if (mode == 1) { // a step of a shadow walk, :341-371
            bool end = true;
            if (hit) {
                shadow *= (1.0f - R.materials[materialOf(S, R, hInst)].alpha);
                ++sCount;
                if (sCount < 4 && shadow > 0.02f) {
                    qo = (qo + qd * hT) + (qd * sBias) * 2.0f;
                    qmin = 0.001f;
                    end = false;
                }
            }
            if (end) {
                if (layer == 0 && phase == 0 && li == 0) aShadow = shadow;
                pending = 1;
                runLights = true;
                mode = 0;
            }
        } else if (!hit) { // :243-245, :398-400, :569-571
            if (phase == 0) done = true;
            else bounceDone = true;
        } else { // a surface: :247-268, :318-321
            sHit = qo + qd * hT;
            sd = qd;
            sBias = fmaxf(0.002f, hT * 0.002f);
            sN = hitNormal<STRIDE>(S, hInst, hPrim, qd);
            sMat = materialOf(S, R, hInst);
            direct = F3{0, 0, 0};
            li = 0;
            pending = 0;
            runLights = true;
            if (phase == 0 && layer == 0) { aInst = hInst; aPrim = (int)hPrim; aDist = hT; }
        }

        if (runLights) { // :322-376 (:473-524, :644-693)
            const sge_render_material& m = R.materials[sMat];
            const F3 V = unit(-sd);
            const float camDist = length(sHit - cam);
            for (int k = 0; k <= nLights; ++k) {
                if (!pending) {
                    if (li >= nLights) { surfaceDone = true; break; }
                    const DevRenderLight& l = R.lights[li];
                    const float NdotL = fmaxf(dot(sN, arr3(l.L)), 0.0f);
                    if (l.enabled < 0.5f || camDist > l.maxDist || !(NdotL > 0.0f)) { ++li; continue; }
                    shadow = 1.0f;
                    if (li == 0 || phase == 2) {
                        qo = sHit + sN * sBias;
                        qd = arr3(l.L);
                        qmin = sBias * 0.5f;
                        qmax = l.maxDist;
                        sCount = 0;
                        mode = 1;
                        break;
                    }
                }
                const DevRenderLight& l = R.lights[li];
                const F3 L = arr3(l.L);
                const float NdotL = fmaxf(dot(sN, L), 0.0f);
                direct = direct + mul(evalBrdf(sN, V, L, arr3(m.baseColor), m.metallic, m.roughness), arr3(l.Li)) * (NdotL * shadow);
                ++li;
                pending = 0;
            }
        }

        if (surfaceDone) { // :378-380 (:525-530, :694-699)
            const sge_render_material& m = R.materials[sMat];
            const F3 ambient = (mul(arr3(m.baseColor), evalEnvSH(sN, F)) * F.ambientIntensity) * m.occlusionStrength;
            const F3 color = (direct + ambient) + arr3(m.emissive);
            if (phase == 0) {
                pHit = sHit; pN = sN; pd = sd; pBias = sBias; pMat = sMat; pColor = color;
                if (m.roughness <= 0.08f && m.metallic >= 0.8f) { // :383-390
                    if (layer == 0) aFlags |= 1;
                    qo = sHit + sN * sBias;
                    qd = sd - sN * (2.0f * dot(sN, sd));
                    rd = qd;
                    qmin = sBias * 0.5f;
                    qmax = 1e6f;
                    phase = 1;
                } else {
                    checkRefraction = true;
                }
            } else {
                bAccum = color * m.alpha;
                bAlpha = m.alpha;
                bounceDone = true;
            }
        }

        if (bounceDone) {
            const sge_render_material& m = R.materials[pMat];
            const float NoV = sat(dot(pN, unit(-pd)));
            if (phase == 1) { // :537-541
                const F3 reflColor = bAccum + bg * (1.0f - bAlpha);
                const F3 F0 = F3{0.04f, 0.04f, 0.04f} + (arr3(m.baseColor) - F3{0.04f, 0.04f, 0.04f}) * m.metallic;
                pColor = mix3(pColor, reflColor, fresnelSchlick(NoV, F0));
                checkRefraction = true;
            } else { // :706-711
                const F3 refrBg = evalEnvSH(rd, F) * F.ambientIntensity;
                const F3 refrColor = bAccum + refrBg * (1.0f - bAlpha);
                const F3 Fr = fresnelSchlick(NoV, F3{0.04f, 0.04f, 0.04f});
                const F3 transColor = mul(refrColor, arr3(m.baseColor));
                const F3 mixColor = mul(transColor, F3{1.0f, 1.0f, 1.0f} - Fr) + mul(pColor, Fr);
                pColor = pColor + (mixColor - pColor) * m.transmission;
                composite = true;
            }
        }

        if (checkRefraction) { // :545-561
            const sge_render_material& m = R.materials[pMat];
            composite = true;
            if (m.transmission > 0.001f) {
                const F3 V = unit(-pd);
                F3 n = pN;
                float eta = 1.0f / m.ior;
                if (dot(n, V) < 0.0f) { n = -n; eta = m.ior; }
                const F3 I = -V;
                const float d = dot(n, I);
                const float k = 1.0f - (eta * eta) * (1.0f - d * d);
                const F3 Tr = k < 0.0f ? F3{0, 0, 0} : I * eta - n * (eta * d + sqrtf(k));
                if (length(Tr) > 0.0f) {
                    if (layer == 0) aFlags |= 2;
                    qo = pHit + Tr * pBias;
                    qd = unit(Tr);
                    rd = qd;
                    qmin = pBias * 0.5f;
                    qmax = 1e6f;
                    phase = 2;
                    composite = false;
                }
            }
        }

        if (composite) { // :715-721
            const float alpha = R.materials[pMat].alpha;
            const float oneMinus = 1.0f - accumAlpha;
            accum = accum + (pColor * alpha) * oneMinus;
            accumAlpha += alpha * oneMinus;
            ++layer;
            if (layer < 3 && accumAlpha < 0.99f) {
                qo = pHit + pd * (pBias * 2.0f);
                qd = pd;
                qmin = 0.001f;
                qmax = 1e6f;
                phase = 0;
            } else {
                done = true;
            }
        }
    }

    if (lane != 0) return;
    // :724-729
    const F3 outColor = accum + bg * (1.0f - accumAlpha);
    const float dither = (hash12((float)gx, (float)gy) - 0.5f) * (1.0f / 255.0f);
    float* o = R.rgba + (size_t)pixel * 4;
    o[0] = fmaxf(outColor.x + dither, 0.0f);
    o[1] = fmaxf(outColor.y + dither, 0.0f);
    o[2] = fmaxf(outColor.z + dither, 0.0f);
    o[3] = 1.0f;
    if (R.aov) R.aov[pixel] = sge_render_aov{layer, aInst, aPrim, aDist, aShadow, accumAlpha, queries, aFlags};
}

void launch_render_frame(const RenderArgs& host, const RenderArgs* d_args, hipStream_t s) {
    const int n = host.R.frame.width * host.R.frame.height;
    if (n <= 0) return;
    if (host.S.crowd && host.S.T.layout == SGE_LAYOUT_PADDED16) hipLaunchKernelGGL((render_frame_kernel<4>), dim3(n), dim3(kWave), 0, s, d_args);
    else hipLaunchKernelGGL((render_frame_kernel<3>), dim3(n), dim3(kWave), 0, s, d_args);
}

} // namespace sge
