// One pixel of the frame: the body of render_frame_kernel (sge_render.hip) and of render_ragged_frame_kernel
// (sge_scene_variants.hip), included inside the kernel (see sge_scene_trace_body.inc for why it is a text and not a function). In
// scope where it is included: STRIDE (floats per vertex of the crowd's skinned positions), the kernel's argument A, C, the
// crowd half's accessor over A->S.T (sge_ray_scene_dev.hpp), and TEX, a constant that depends on STRIDE (so that the arm of an
// `if constexpr (TEX)` that is not taken is discarded unseen): true in the textured kernels (include/sge_amd_render_textures.h),
// which sample where the text samples and carry the sampled surface; false in the kernels of sge_amd_render.h, which compile to
// what they were. IBL, a constant of the same kind: true in the kernels of include/sge_amd_render_ibl.h, which add eval_spec_ibl
// to the colour of the layer's own surface.
    __shared__ int stack[kBlasStack];
    const int lane = threadIdx.x;
    // (the two records are read where they are used, from device memory: as kernel arguments they were held in scalar registers
    // across the whole loop, more of them than there are)
    const SceneTrace& S = A->S;
    const RenderLaunch& R = A->R;
    const sge_render_frame& F = R.frame;
    const BlasTrace& T = S.T;
    const RenderTextures& X = A->X; // (read by the textured form only)
    const RenderIBL& E = A->I;      // (read by the IBL forms only)
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
    __shared__ PixelStateT<TEX> ps;
    // the layer's surface once shaded, kept while a bounce is shaded
    F3 &pHit = ps.pHit, &pN = ps.pN, &pd = ps.pd, &pColor = ps.pColor;
    float& pBias = ps.pBias;
    // the surface being shaded
    F3 &sHit = ps.sHit, &sN = ps.sN, &sd = ps.sd, &direct = ps.direct, &rd = ps.rd;
    float &sBias = ps.sBias, &shadow = ps.shadow;
    int &li = ps.li, &sCount = ps.sCount, &pending = ps.pending;
    // the pixel
    F3& accum = ps.accum;
    float& accumAlpha = ps.accumAlpha;
    int &layer = ps.layer, &queries = ps.queries, &phase = ps.phase;
    int &aInst = ps.aInst, &aPrim = ps.aPrim, &aFlags = ps.aFlags;
    float &aDist = ps.aDist, &aShadow = ps.aShadow;
    pHit = F3{0, 0, 0}; pN = F3{0, 0, 1}; pd = dir; pColor = F3{0, 0, 0}; pBias = 0;
    if constexpr (TEX) ps.pSurf = R.materials[0]; else ps.pMat = 0;
    sHit = F3{0, 0, 0}; sN = F3{0, 0, 1}; sd = dir; direct = F3{0, 0, 0}; rd = dir; sBias = 0; shadow = 1.0f;
    if constexpr (TEX) ps.sSurf = R.materials[0]; else ps.sMat = 0;
    li = 0; sCount = 0; pending = 0;
    accum = F3{0, 0, 0}; accumAlpha = 0; layer = 0; queries = 0; phase = 0;
    aInst = -1; aPrim = -1; aFlags = 0; aDist = 0; aShadow = 1.0f;

    BlasBest best{qmax, 0, 0, 0u, -1};
    auto visitStatic = [&](int s) {
        blasTraverseClosest<3, true>(stack, lane, sceneTree(S.meshes[S.meshOf[s]]), loadInstance(S.matrices, s), qo, qd, fmaxf(qmin, 0.0f), qmax,
                                     SGE_SCENE_STATIC_BASE + s, best);
        return false;
    };
    auto visitCharacter = [&](int inst) {
        const int v = C.record(inst);
        if (v == kSceneNoVariant) return false;
        blasTraverseClosest<STRIDE, true>(stack, lane, C.tree(inst, v), loadInstance(T.instances, inst), qo, qd, fmaxf(qmin, 0.0f), qmax, inst, best);
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
                if constexpr (TEX) shadow *= (1.0f - sampleAlpha<STRIDE>(S, R, X, C, hInst, hPrim, uniformFloat(best.u), uniformFloat(best.v), qd)); // sample_alpha, :357
                else shadow *= (1.0f - R.materials[materialOf(S, R, hInst)].alpha);
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
            sN = hitNormal<STRIDE>(S, C, hInst, hPrim, qd);
            if constexpr (TEX) { // sample_material and the normal map, :273-316
                sge_render_material sm;
                F3 n = sN;
                sampleSurface<STRIDE>(S, R, X, C, hInst, hPrim, uniformFloat(best.u), uniformFloat(best.v), qd, sm, n);
                ps.sSurf = sm;
                sN = n;
            } else {
                ps.sMat = materialOf(S, R, hInst);
            }
            direct = F3{0, 0, 0};
            li = 0;
            pending = 0;
            runLights = true;
            if (phase == 0 && layer == 0) { aInst = hInst; aPrim = (int)hPrim; aDist = hT; }
        }

        if (runLights) { // :322-376 (:473-524, :644-693)
            const sge_render_material& m = surfaceS(ps, R);
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
            const sge_render_material& m = surfaceS(ps, R);
            const F3 ambient = (mul(arr3(m.baseColor), evalEnvSH(sN, F)) * F.ambientIntensity) * m.occlusionStrength;
            F3 color;
            if constexpr (IBL) { // :379-380: eval_spec_ibl, at the layer's own surface only
                F3 lit = direct + ambient;
                if (phase == 0) lit = lit + evalSpecIbl(E, sN, unit(-sd), m.roughness, m.metallic, arr3(m.baseColor)) * m.occlusionStrength;
                color = lit + arr3(m.emissive);
            } else {
                color = (direct + ambient) + arr3(m.emissive);
            }
            if (phase == 0) {
                pHit = sHit; pN = sN; pd = sd; pBias = sBias; pColor = color;
                if constexpr (TEX) ps.pSurf = ps.sSurf; else ps.pMat = ps.sMat;
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
            const sge_render_material& m = surfaceP(ps, R);
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
            const sge_render_material& m = surfaceP(ps, R);
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
            const float alpha = surfaceP(ps, R).alpha;
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
