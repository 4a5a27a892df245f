// sge::IBLResources and sge::RayTracingRenderer::setIBL / clearIBL (host/sge_host.hpp, include/sge_amd_render_ibl.h). Without a
// device: the default resources are built on the host and checked against IBLResources.swift's own numbers. On a GPU: a rough
// metal ground seen from above, ambient only; with the environment set the centre pixel gains prefiltered * (F0 * brdf.x + brdf.y)
// computed from the samplers alone; clearIBL gives the first image back.
#include <cmath>
#include <cstdio>
#include "../../swift-game-engine_amd/host/sge_host.hpp"

static int fail(const char* what) { std::printf("FAILED: %s (%s)\n", what, sge_last_error()); return 1; }

int main() {
    // needs no device: a small pair, then the shapes of the defaults (128 / 128 / 256 samples)
    try {
        const sge::IBLResources small(4, 4, 16);
        if (small.envMipCount != 3 || small.envCube.size() != 6 * (16 + 4 + 1) * 4 || small.brdfLUT.size() != 4 * 4 * 4) return fail("IBLResources(4, 4, 16)");
        if (small.envCube[3] != 0x3C00) return fail("alpha is the half 1.0");
        if (!(small.brdfLUT[4 * 15] > 0.0f && small.brdfLUT[4 * 15] < 1.0f) || small.brdfLUT[4 * 15 + 2] != 0.0f) return fail("the table's corner");
        bool threw = false;
        try { const sge::IBLResources bad(3, 4, 16); } catch (const sge::Error&) { threw = true; }
        if (!threw) return fail("a cube size that is no power of two is refused");
    } catch (const sge::Error& e) { return fail(e.what()); }
    const sge::IBLResources ibl;
    if (ibl.envSize != 128 || ibl.envMipCount != 8 || ibl.lutSize != 128 || ibl.brdfLUT.size() != 128 * 128 * 4) return fail("the default IBLResources");
    size_t texels = 0;
    for (int m = 0; m < 8; ++m) texels += 6 * (size_t)(128 >> m) * (128 >> m);
    if (ibl.envCube.size() != texels * 4) return fail("the default cube's chain");

    auto world = sge::World::make(0);
    if (!world) { std::printf("no device: render ibl smoke skipped the GPU part\n"); return 2; }
    sge_context* ctx = world->context();
    const float pos[12] = {-4, 0, -4, 4, 0, -4, 4, 0, 4, -4, 0, 4};
    const float nrm[12] = {0, 1, 0, 0, 1, 0, 0, 1, 0, 0, 1, 0};
    const float tan[16] = {1, 0, 0, 1, 1, 0, 0, 1, 1, 0, 0, 1, 1, 0, 0, 1};
    const uint32_t idx[6] = {0, 2, 1, 0, 3, 2};
    if (sge_scene_mesh_upload(ctx, 0, pos, nrm, tan, nullptr, 4, idx, 6) != SGE_OK) return fail("sge_scene_mesh_upload");
    const int32_t meshOf[1] = {0};
    const float identity[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    if (sge_scene_instances_set(ctx, 1, meshOf, identity) != SGE_OK) return fail("sge_scene_instances_set");
    const float view[16] = {1, 0, 0, 0, 0, 0, 1, 0, 0, -1, 0, 0, 0, 0, -5, 1};
    const float t = 1.0f / std::tan(0.2f), n = 0.1f, f = 100.0f;
    const float proj[16] = {t, 0, 0, 0, 0, t, 0, 0, 0, 0, f / (n - f), -1, 0, 0, f * n / (n - f), 0};
    const float cam[3] = {0, 5, 0};
    sge::RayTracingRenderer renderer(*world);
    float plain[3 * 3 * 4], lit[3 * 3 * 4], cleared[3 * 3 * 4];
    try {
        sge_render_material metal{};
        metal.baseColor[0] = 0.9f; metal.baseColor[1] = 0.8f; metal.baseColor[2] = 0.7f;
        metal.metallic = 1.0f; metal.roughness = 0.4f; metal.alpha = 1.0f; metal.occlusionStrength = 1.0f; metal.ior = 1.5f;
        renderer.setMaterials({metal});
        renderer.encode(3, 3, {}, cam, proj, view, plain);
        int32_t size = -1, mips = -1, lw = -1, lh = -1;
        renderer.iblInfo(size, mips, lw, lh);
        if (size != 0 || mips != 0 || lw != 0 || lh != 0) return fail("a fresh context has no environment");
        renderer.setIBL(ibl);
        renderer.iblInfo(size, mips, lw, lh);
        if (size != 128 || mips != 8 || lw != 128 || lh != 128) return fail("iblInfo after setIBL");
        renderer.encode(3, 3, {}, cam, proj, view, lit);
        // the centre pixel looks straight down: N = V = R = +Y, NoV = 1, mip = 0.4 * 7
        const std::vector<float> pre = renderer.sampleEnvironment({0, 1, 0}, {0.4f * 7.0f});
        const std::vector<float> brdf = renderer.sampleBrdfLUT({1.0f, 0.4f});
        for (int k = 0; k < 3; ++k) {
            const float F0 = 0.04f + (metal.baseColor[k] - 0.04f) * 1.0f;
            const float spec = pre[k] * (F0 * brdf[0] + brdf[1]);
            if (!(spec > 0.05f)) return fail("the sky reflects in a rough metal");
            if (std::fabs((lit[4 * 4 + k] - plain[4 * 4 + k]) - spec) > 2e-5f) return fail("the centre pixel gains eval_spec_ibl");
        }
        renderer.clearIBL();
        renderer.encode(3, 3, {}, cam, proj, view, cleared);
    } catch (const sge::Error& e) { return fail(e.what()); }
    for (int k = 0; k < 3 * 3 * 4; ++k)
        if (cleared[k] != plain[k]) return fail("clearIBL gives the frame without the term back");
    std::printf("render ibl smoke ok\n");
    return 0;
}
