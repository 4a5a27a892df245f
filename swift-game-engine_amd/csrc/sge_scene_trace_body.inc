// The closest hit of one ray in both halves with the reads at the hit: the body of scene_trace_kernel (sge_ray_scene.hip) and of
// scene_ragged_trace_kernel (sge_scene_variants.hip), included inside the kernel. One text, not a function: as a function taking the
// launch record, the uniform kernels no longer compiled to what this text compiles to in place. In scope where it is included:
// STRIDE (floats per vertex of the crowd's skinned positions and normals; the static meshes' streams are packed), the kernel's
// arguments S, rays, n, hits, and C, the crowd half's accessor over S.T (sge_ray_scene_dev.hpp).
    __shared__ int stack[kBlasStack];
    const int lane = threadIdx.x;
    if ((int)blockIdx.x >= n) return;
    const sge_blas_ray R = rays[blockIdx.x];
    const BlasTrace& T = S.T;
    const F3 wo{R.origin[0], R.origin[1], R.origin[2]}, wd{R.direction[0], R.direction[1], R.direction[2]};
    const float tMin = smax(R.minDistance, 0.0f);
    BlasBest best{R.maxDistance, 0, 0, 0u, -1};

    auto visitStatic = [&](int s) {
        blasTraverseClosest<3, true>(stack, lane, sceneTree(S.meshes[S.meshOf[s]]), loadInstance(S.matrices, s), wo, wd, tMin, R.maxDistance,
                               SGE_SCENE_STATIC_BASE + s, best);
        return false;
    };
    auto visitCharacter = [&](int inst) {
        const int v = C.record(inst);
        if (v == kSceneNoVariant) return false;
        blasTraverseClosest<STRIDE, true>(stack, lane, C.tree(inst, v), loadInstance(T.instances, inst), wo, wd, tMin, R.maxDistance, inst, best);
        return false;
    };

    // a ray names one instance (a scene id) or asks both halves; an id that names nothing enters neither scan
    const F3 inv = invDir(wd);
    const int id = R.instance, sOnly = id >= SGE_SCENE_STATIC_BASE ? id - SGE_SCENE_STATIC_BASE : -1;
    if (S.statics > 0 && (id < 0 || (sOnly >= 0 && sOnly < S.statics)))
        sceneScan(S.boxes, S.boxes + (size_t)S.statics * 6, nullptr, nullptr, S.statics, sOnly, lane, wo, inv, tMin, best.t, visitStatic);
    // (a named character is walked directly: routed through the scan as the statics are, the kernel spilled scalar registers)
    if (S.crowd && id >= 0) {
        if (id < T.chars) visitCharacter(id);
    } else if (S.crowd) {
        const int* order = T.instOrder; // null: the flat form (SGE_BLAS_FLAT_INSTANCES)
        sceneScan(T.worldBoxes, order ? T.groupBoxes : T.worldBoxes + (size_t)T.chars * 6, order ? T.superBoxes : nullptr, order, T.chars, -1, lane,
                  wo, inv, tMin, best.t, visitCharacter);
    }
    if (lane != 0) return;
    sge_blas_hit H{};
    H.primitive = -1;
    H.instance = -1;
    if (best.inst >= SGE_SCENE_STATIC_BASE) {
        const int s = best.inst - SGE_SCENE_STATIC_BASE;
        const DevSceneMesh& m = S.meshes[S.meshOf[s]];
        blasHitRecord<3>(loadInstance(S.matrices, s), m.positions, m.normals, m.tangents, m.uvs, m.indices + (size_t)best.prim * 3, wd, best, H);
        H.instance = best.inst;
    } else if (best.inst >= 0) {
        const CrowdStreams cs = C.streams(best.inst);
        const size_t vbase = cs.vbase;
        blasHitRecord<STRIDE>(loadInstance(T.instances, best.inst), reinterpret_cast<const float*>(T.positions) + vbase * STRIDE,
                              reinterpret_cast<const float*>(T.normals) + vbase * STRIDE, T.tangents + vbase * 4, cs.uvs,
                              cs.indices + (size_t)best.prim * 3, wd, best, H);
        H.instance = best.inst;
    }
    hits[blockIdx.x] = H;
