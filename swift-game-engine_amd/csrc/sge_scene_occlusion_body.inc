// Is anything between minDistance and maxDistance? The body of scene_occlusion_kernel (sge_ray_scene.hip) and of
// scene_ragged_occlusion_kernel (sge_scene_variants.hip), included inside the kernel (see sge_scene_trace_body.inc). In scope where it
// is included: STRIDE, the kernel's arguments S, rays, n, occluded, and C, the crowd half's accessor over S.T.
    __shared__ int stack[kBlasStack];
    const int lane = threadIdx.x;
    if ((int)blockIdx.x >= n) return;
    const sge_blas_ray R = rays[blockIdx.x];
    const BlasTrace& T = S.T;
    const F3 wo{R.origin[0], R.origin[1], R.origin[2]}, wd{R.direction[0], R.direction[1], R.direction[2]};
    const float tMin = smax(R.minDistance, 0.0f);
    const float bound = R.maxDistance;

    auto visitStatic = [&](int s) {
        return sceneOccludedOne<3>(stack, lane, sceneTree(S.meshes[S.meshOf[s]]), loadInstance(S.matrices, s), wo, wd, tMin, bound);
    };
    auto visitCharacter = [&](int inst) {
        const int v = C.record(inst);
        if (v == kSceneNoVariant) return false;
        return sceneOccludedOne<STRIDE>(stack, lane, C.tree(inst, v), loadInstance(T.instances, inst), wo, wd, tMin, bound);
    };

    bool occ = false;
    const F3 inv = invDir(wd);
    const int id = R.instance, sOnly = id >= SGE_SCENE_STATIC_BASE ? id - SGE_SCENE_STATIC_BASE : -1;
    if (S.statics > 0 && (id < 0 || (sOnly >= 0 && sOnly < S.statics)))
        occ = sceneScan(S.boxes, S.boxes + (size_t)S.statics * 6, nullptr, nullptr, S.statics, sOnly, lane, wo, inv, tMin, bound, visitStatic);
    if (!occ && S.crowd && id < T.chars && T.chars > 0) {
        const int* order = id < 0 ? T.instOrder : nullptr;
        occ = sceneScan(T.worldBoxes, order ? T.groupBoxes : T.worldBoxes + (size_t)T.chars * 6, order ? T.superBoxes : nullptr, order, T.chars, id, lane,
                        wo, inv, tMin, bound, visitCharacter);
    }
    if (lane == 0) occluded[blockIdx.x] = occ ? 1 : 0;
