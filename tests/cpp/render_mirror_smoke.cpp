// sge::RayTracingRenderer (host/sge_host.hpp) on a GPU: a ground quad seen from above, rendered through encode() with an empty light
// list (the reference's quirk: a default light is uploaded, dirLightCount stays 0, the pixel is ambient only) and with one light.
#include <cmath>
#include <cstdio>
#include "../../swift-game-engine_amd/host/sge_host.hpp"

static int fail(const char* what) { std::printf("FAILED: %s (%s)\n", what, sge_last_error()); return 1; }

int main() {
    // inverse4 needs no device
    const float m[16] = {2, 0, 0, 0, 0, 3, 0, 0, 1, 0, 0.5f, -1, 4, 5, 6, 1};
    float inv[16];
    if (!sge::RayTracingRenderer::inverse4(m, inv)) return fail("inverse4");
    for (int c = 0; c < 4; ++c)
        for (int r = 0; r < 4; ++r) {
            float a = 0;
            for (int k = 0; k < 4; ++k) a += m[k * 4 + r] * inv[c * 4 + k];
            if (std::fabs(a - (r == c ? 1.0f : 0.0f)) > 1e-5f) return fail("inverse4 * m != identity");
        }
    float none[16];
    const float singular[16] = {1, 0, 0, 0, 2, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    if (sge::RayTracingRenderer::inverse4(singular, none)) return fail("a singular matrix has no inverse");

    auto world = sge::World::make(0);
    if (!world) { std::printf("no device: render mirror smoke skipped the GPU part\n"); return 2; }
    sge_context* ctx = world->context();
    const float pos[12] = {-4, 0, -4, 4, 0, -4, 4, 0, 4, -4, 0, 4};
    const float nrm[12] = {0, 1, 0, 0, 1, 0, 0, 1, 0, 0, 1, 0};
    const float tan[16] = {1, 0, 0, 1, 1, 0, 0, 1, 1, 0, 0, 1, 1, 0, 0, 1};
    const uint32_t idx[6] = {0, 2, 1, 0, 3, 2};
    if (sge_scene_mesh_upload(ctx, 0, pos, nrm, tan, nullptr, 4, idx, 6) != SGE_OK) return fail("sge_scene_mesh_upload");
    const int32_t meshOf[1] = {0};
    const float identity[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    if (sge_scene_instances_set(ctx, 1, meshOf, identity) != SGE_OK) return fail("sge_scene_instances_set");

    // a camera at (0, 5, 0) looking down, up = -z: view rows (1,0,0), (0,0,-1), (0,1,0); column-major
    const float view[16] = {1, 0, 0, 0, 0, 0, 1, 0, 0, -1, 0, 0, 0, 0, -5, 1};
    const float t = 1.0f / std::tan(0.2f), n = 0.1f, f = 100.0f;
    const float proj[16] = {t, 0, 0, 0, 0, t, 0, 0, 0, 0, f / (n - f), -1, 0, 0, f * n / (n - f), 0};
    const float cam[3] = {0, 5, 0};
    sge::RayTracingRenderer renderer(*world);
    float dark[3 * 3 * 4], lit[3 * 3 * 4];
    sge_render_aov aov[9];
    try {
        renderer.encode(3, 3, {}, cam, proj, view, dark, aov);
        if (aov[4].instance != SGE_SCENE_STATIC_BASE || std::fabs(aov[4].distance - 5.0f) > 1e-4f || aov[4].queries != 1) return fail("the centre pixel sees the quad; no light, no shadow ray");
        sge::DirectionalLight sun;
        sun.direction[0] = 0; sun.direction[1] = -1; sun.direction[2] = 0;
        renderer.encode(3, 3, {sun}, cam, proj, view, lit, aov);
        if (aov[4].queries != 2 || aov[4].shadow != 1.0f) return fail("one light: the layer's ray and one shadow ray that misses");
    } catch (const sge::Error& e) { return fail(e.what()); }
    // ambient only: base 1 * (envSH0 * c0 + envSH1 * c1 * N.y) * 0.25 = ((sky + ground) / 2 + (sky - ground) / 2) / 4 = sky / 4, +- the dither
    const float sky[3] = {0.7f, 0.8f, 1.0f};
    for (int k = 0; k < 3; ++k)
        if (std::fabs(dark[4 * 4 + k] - sky[k] * 0.25f) > 0.5f / 255.0f + 1e-5f) return fail("empty light list: ambient only");
    // + brdf (1.16 / pi, N = V = L) * Li (2.6 * color)
    const float color[3] = {1.0f, 0.95f, 0.85f};
    for (int k = 0; k < 3; ++k)
        if (std::fabs((lit[4 * 4 + k] - dark[4 * 4 + k]) - 1.16f / 3.14159265f * 2.6f * color[k]) > 1e-4f) return fail("one light straight above");
    std::printf("render mirror smoke ok\n");
    return 0;
}
