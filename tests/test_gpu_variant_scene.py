"""A crowd with mesh variants in the ray scene and the shaded frame (include/sge_amd_variant_scene.h; csrc/sge_scene_variants.hip)
on the GPU.

The world is that of tests/test_gpu_variant_blas.py (65 bones, 37 characters, both output layouts, four variants of (9001, 9000),
(1001, 1200), (3, 1) and (300, 500) vertices and triangles, its assignment patterns), with three static meshes in six instances
beside it: a plane behind the crowd; a small quad in front of two characters' targets, between two characters and away from everything; one
triangle that is an exact world-space copy of a triangle of character 0 (whose instance matrix is the identity), so that both
halves report the same distance bits. Every ray direction has three non-zero components. (The synthetic characters are some 350
units across and stand 35 apart: they overlap, so a ray usually meets other triangles before the one it is aimed at.)

References: sge_blas_intersect_batch on the same context (pinned bit for bit to uniform contexts by test_gpu_variant_blas.py) for a
ray that names a character; compose([the same rays on a context that holds the statics only, sge_blas_intersect_batch(-1)]) for a
whole-scene ray, byte for byte; SceneRef over the CPU oracle with VariantCrowdRef (tests/variant_scene_ref.py) within the bars of
scene_ref.assert_records_match; a uniform context for the frame."""
import ctypes as C

import numpy as np
import pytest

from scene_ref import STATIC_BASE, SceneRef, assert_records_match, columns, compose
from test_gpu_ray_scene import _dress, _upload
from test_gpu_variant_blas import CHARS, NV, SHAPES, TICKS, _Ctx, _cols, _hip, _instances, _mesh, _palettes, _patterns, _rig, _scene_ctx
from variant_scene_ref import VariantCrowdRef

pytestmark = pytest.mark.gpu

DIRS = np.array([[0.21, -0.33, 0.92], [-0.4, 0.25, 0.88], [0.15, 0.5, 0.85]], np.float32)
DIRS /= np.linalg.norm(DIRS, axis=1, keepdims=True)
FAR = 60.0  # a ray starts this far in front of its target


def _world_positions(ctx):
    """Per character the world positions of its vertices, from the ragged stream of the newest launch (float32, the kernels' bytes
    for a character whose instance matrix is the identity)."""
    off = ctx.eng.vertex_offsets()
    pos = ctx.eng.skinned(0, int(off[-1]))[0]
    M = _instances()
    out = []
    for c in range(CHARS):
        p = pos[off[c]:off[c + 1]]
        out.append(p if np.array_equal(M[c], np.eye(4, dtype=np.float32)) else (p @ M[c][:3, :3].T + M[c][:3, 3]).astype(np.float32))
    return out


def _pick_tie(ctx, world, assign):
    """A triangle of character 0 that the crowd alone reports for the windowed ray at its centroid (the characters overlap: most
    triangles have another one within the window)."""
    tris = _mesh(int(assign[0]))["indices"].reshape(-1, 3)
    cand = np.arange(0, len(tris), 97)[:64]
    tgt = np.stack([world[0][tris[k]].astype(np.float64).mean(0) for k in cand]).astype(np.float32)
    d = np.tile(DIRS[0], (len(cand), 1))
    h = ctx.eng.blas_intersect(tgt - d * FAR, d, np.full(len(cand), -1, np.int32), min_distance=FAR - 0.05, max_distance=1e6)
    ok = np.flatnonzero((h["hit"] == 1) & (h["instance"] == 0) & (h["primitive"] == cand))
    assert len(ok), "no candidate triangle of character 0 is alone in its window"
    return int(cand[ok[0]])


def _statics(world, assign, tie_prim):
    """(meshes {id: dict}, mesh_of [6], mats [6][4][4] row-major)."""
    allp = np.concatenate(world)
    lo, hi = allp.min(0), allp.max(0)
    z = float(hi[2] + 40)
    plane = _dress(np.array([[lo[0] - 80, lo[1] - 80, z], [hi[0] + 80, lo[1] - 80, z], [hi[0] + 80, hi[1] + 80, z], [lo[0] - 80, hi[1] + 80, z]], np.float32),
                   [0, 1, 2, 0, 2, 3], 21)
    quad = _dress(np.array([[-3, -3, 0], [3, -3, 0], [3, 3, 0], [-3, 3, 0], [0, 0, 1.5]], np.float32), [0, 1, 2, 0, 2, 3, 0, 1, 4], 22)
    tri0 = _mesh(int(assign[0]))["indices"].reshape(-1, 3)[tie_prim]
    tie = _dress(world[0][tri0].copy(), [0, 1, 2], 23)
    mats = np.tile(np.eye(4, dtype=np.float32), (6, 1, 1))
    for slot, c in ((1, 3), (2, 12)):  # in front of characters 3 and 12 on the rays' side
        t = _mesh(int(assign[c]))["indices"].reshape(-1, 3)[0]
        mats[slot][:3, 3] = world[c][t].mean(0) - DIRS[0] * 9.0
    mats[3][:3, 3] = (world[8].mean(0) + world[9].mean(0)) / 2
    mats[4][:3, 3] = (lo[0] - 400, hi[1] + 500, lo[2] - 300)
    return {0: plane, 1: quad, 2: tie}, np.array([0, 1, 1, 1, 1, 2], np.int32), mats


def _set_statics(eng, meshes, mesh_of, mats):
    for k, m in meshes.items():
        _upload(eng, k, m)
    eng.scene_instances(mesh_of, columns(mats))


def _rays(world, assign, mats, tie_prim, seed=4):
    """-> origins, directions, character aimed at (-1: none), min distances, max distances. The last ray is the tie ray."""
    rng = np.random.default_rng(seed)
    O, D, I, lo, hi = [], [], [], [], []

    def add(target, d, c=-1, mn=0.001, mx=1e6):
        O.append(np.asarray(target, np.float32) - d * FAR); D.append(d); I.append(c); lo.append(mn); hi.append(mx)

    for c in range(CHARS):
        tris = _mesh(int(assign[c]))["indices"].reshape(-1, 3)
        for k, t in enumerate(tris[rng.integers(0, len(tris), 3)]):
            add(world[c][t].mean(0), DIRS[k], c)
        t = tris[0]
        add(world[c][t].mean(0), DIRS[0], c, mx=FAR * 0.5)   # the window ends in front of the character
        add(world[c][t].mean(0), DIRS[1], c, mn=FAR * 1.5)   # the window starts behind the target
    for s in range(6):                                       # at the statics
        add(mats[s][:3, 3] + (0.3, 0.2, 0.0), DIRS[s % 3])
    allp = np.concatenate(world)
    add(allp.max(0) + (900, 900, -200), DIRS[2])             # past everything
    add(allp.min(0) - (900, 900, 200), -DIRS[1])
    for c in np.flatnonzero(assign == 2):                    # the one-triangle variant, alone in its window
        add(world[c][:3].astype(np.float64).mean(0), DIRS[2], c, mn=FAR - 0.05)
    for c in (3, 12):                                        # through the quad that stands 9 in front of the target, from just before it (the crowd is dense: a wider window meets a character first)
        t = _mesh(int(assign[c]))["indices"].reshape(-1, 3)[0]
        add(world[c][t].mean(0), DIRS[0], c, mn=FAR - 9.01)
    tri0 = _mesh(int(assign[0]))["indices"].reshape(-1, 3)[tie_prim]
    add(world[0][tri0].astype(np.float64).mean(0), DIRS[0], 0, mn=FAR - 0.05)  # the tie ray: nothing in front of its target counts
    return (np.array(O, np.float32), np.array(D, np.float32), np.array(I, np.int32), np.array(lo, np.float32), np.array(hi, np.float32))


def _same_bytes(a, b, what):
    for f in a.dtype.names:
        same = a[f].view(np.uint32 if a[f].dtype.itemsize == 4 else np.uint8) == b[f].view(np.uint32 if b[f].dtype.itemsize == 4 else np.uint8)
        assert same.all(), (what, f, np.argwhere(~same)[:5].tolist(), a[f][~same][:5], b[f][~same][:5])


@pytest.fixture(scope="module", params=["packed", "padded16"])
def scene(sge, request):
    """(variant context with the statics, context with the statics only, assignment, world positions, statics, rays)"""
    ctx = _Ctx(sge, request.param, range(NV))
    only = sge.CharacterEngine(0)
    try:
        ctx.write_palettes(_palettes())
        assign = _patterns()["mixed"]
        ctx.eng.set_mesh_variants(assign)
        ctx.tick()
        world = _world_positions(ctx)
        tie_prim = _pick_tie(ctx, world, assign)
        meshes, mesh_of, mats = _statics(world, assign, tie_prim)
        _set_statics(ctx.eng, meshes, mesh_of, mats)
        _set_statics(only, meshes, mesh_of, mats)
        yield ctx, only, assign, world, (meshes, mesh_of, mats, tie_prim), _rays(world, assign, mats, tie_prim)
    finally:
        ctx.eng.close()
        only.close()


def _retick(ctx, assign):
    ctx.eng.reserve_vertices(0)
    ctx.eng.set_mesh_variants(assign)
    ctx.tick()


def _expected_whole(ctx, only, O, D, mn, mx):
    n = len(O)
    statics = only.scene_intersect(O, D, np.full(n, -1, np.int32), mn, mx)
    crowd = ctx.eng.blas_intersect(O, D, np.full(n, -1, np.int32), min_distance=mn, max_distance=mx)
    return compose([statics, crowd]), statics, crowd


def test_named_characters_are_the_records_of_blas_intersect(scene):
    ctx, only, assign, world, _, (O, D, I, mn, mx) = scene
    _retick(ctx, assign)
    st = ctx.eng.scene_crowd_status()
    assert (st.crowdReady, st.ragged, st.reason, st.variant) == (1, 1, ctx.A.SCENE_CROWD_OK, -1)
    sel = I >= 0
    got = ctx.eng.scene_intersect(O[sel], D[sel], I[sel], mn[sel], mx[sel])
    want = ctx.eng.blas_intersect(O[sel], D[sel], I[sel], min_distance=mn[sel], max_distance=mx[sel])
    _same_bytes(got, want, "named characters")
    full = (mn[sel] < 1) & (mx[sel] > 1e5)
    assert (got["hit"][full] == 1).all() and (got["instance"][full] == I[sel][full]).all(), "a ray at a triangle's centroid hits its character"
    for v in range(NV):
        of_v = full & (assign[I[sel]] == v)
        assert of_v.any() and (got["primitive"][of_v] < SHAPES[v][1]).all(), "a triangle of the variant's own index buffer"
    assert (got["distance"][full] <= FAR * 1.001).all()
    cut = got["hit"] == 1
    assert (got["distance"][cut] <= mx[sel][cut]).all() and (got["distance"][cut] >= mn[sel][cut]).all(), "hits stay inside their window"
    assert np.array_equal(ctx.eng.scene_occluded(O[sel], D[sel], I[sel], mn[sel], mx[sel]), got["hit"])


def test_whole_scene_rays_compose_the_two_halves(sge, scene):
    ctx, only, assign, world, (meshes, mesh_of, mats, tie_prim), (O, D, I, mn, mx) = scene
    _retick(ctx, assign)
    n = len(O)
    got = ctx.eng.scene_intersect(O, D, np.full(n, -1, np.int32), mn, mx)
    want, statics, crowd = _expected_whole(ctx, only, O, D, mn, mx)
    _same_bytes(got, want, "whole-scene rays")
    assert (got["instance"] >= STATIC_BASE).any() and ((got["instance"] >= 0) & (got["instance"] < CHARS)).any() and (got["hit"] == 0).any()
    for v in range(NV):  # (variant 2, one triangle inside the mass of its neighbours, through the windowed rays at it)
        assert (assign[got["instance"][(got["hit"] == 1) & (got["instance"] < CHARS)]] == v).any(), ("no hit on variant", v)
    # a static instance in front of a character takes the hit from it: the quads before characters 3 and 12
    front = got["instance"][-3:-1]
    print("quads in front of characters 3 and 12 report", front.tolist(), "distances", got["distance"][-3:-1].tolist())
    assert (front == np.array([STATIC_BASE + 1, STATIC_BASE + 2])).any(), front.tolist()
    # the tie: the static copy and the character report the same distance bits, the character takes the hit
    assert statics["hit"][-1] == 1 and statics["instance"][-1] == STATIC_BASE + 5 and crowd["hit"][-1] == 1 and crowd["instance"][-1] == 0
    assert statics["distance"][-1:].view(np.uint32)[0] == crowd["distance"][-1:].view(np.uint32)[0], "the halves tie"
    assert got["instance"][-1] == 0 and got["primitive"][-1] == tie_prim
    assert np.array_equal(ctx.eng.scene_occluded(O, D, np.full(n, -1, np.int32), mn, mx), got["hit"])
    # ids that name nothing
    ids = np.array([CHARS, CHARS + 5, STATIC_BASE + 6, STATIC_BASE + 100, 2 ** 31 - 1], np.int32)
    k = len(ids)
    g = ctx.eng.scene_intersect(O[:k], D[:k], ids)
    assert (g["hit"] == 0).all() and (g["instance"] == -1).all()
    assert (ctx.eng.scene_occluded(O[:k], D[:k], ids) == 0).all()
    # the CPU oracle: one engine per variant over the GPU's ragged streams
    off = ctx.eng.vertex_offsets()
    p, nr, tn = ctx.eng.skinned(0, int(off[-1]))
    _, rec = ctx.eng.blas_variant_bounds()
    vm = [dict(_mesh(v), tangents=np.tile(np.array([1, 0, 0, 1], np.float32), (SHAPES[v][0], 1))) for v in range(NV)]
    crowd_ref = VariantCrowdRef(sge, vm, rec, off, p, nr, tn, _cols(_instances()))
    ref = SceneRef(sge, meshes, mesh_of, mats, crowd=crowd_ref)
    try:
        keep = np.arange(n - 1)  # (the tie ray is decided by bits the float64-free oracle need not share)
        w = ref.intersect(O[keep], D[keep], -1, mn[keep], mx[keep])
        assert_records_match(got[keep], w, "whole scene against the oracle")
        named = I[keep] >= 0
        w = ref.intersect(O[keep][named], D[keep][named], I[keep][named], mn[keep][named], mx[keep][named])
        assert_records_match(ctx.eng.scene_intersect(O[keep][named], D[keep][named], I[keep][named], mn[keep][named], mx[keep][named]), w, "named against the oracle")
    finally:
        ref.close()
        crowd_ref.close()


def test_records_decide_who_is_in_the_scene(scene):
    ctx, only, assign, world, _, (O, D, I, mn, mx) = scene
    eng, A = ctx.eng, ctx.A
    n = len(O)
    whole = np.full(n, -1, np.int32)
    counts = np.array([SHAPES[v][0] for v in assign], np.int64)
    off = np.concatenate([[0], np.cumsum(counts)])
    k = int(np.flatnonzero(assign[20:] == 0)[0]) + 20
    statics_only = only.scene_intersect(O, D, whole, mn, mx)
    try:
        for what, capacity in (("inside a slice", int(off[k]) + 5), ("on a boundary", int(off[k]))):
            kept = off[1:] <= capacity
            assert 0 < kept.sum() < CHARS and not kept[k] and kept[k - 1]
            eng.reserve_vertices(capacity)
            eng.set_mesh_variants(assign)
            ctx.tick()
            assert eng.skin_plan().dropped == CHARS - kept.sum()
            _, rec = eng.blas_variant_bounds()
            assert np.array_equal(rec, np.where(kept, assign, A.NO_VARIANT)), what
            assert eng.scene_crowd_status().crowdReady == 1 and eng.scene_info().crowdReady == 1
            sel = I >= 0
            g = eng.scene_intersect(O[sel], D[sel], I[sel], mn[sel], mx[sel])
            dropped = ~kept[I[sel]]
            assert dropped.any() and (g["hit"][dropped] == 0).all() and (g["instance"][dropped] == -1).all(), what
            _same_bytes(g, eng.blas_intersect(O[sel], D[sel], I[sel], min_distance=mn[sel], max_distance=mx[sel]), what)
            occ = eng.scene_occluded(O[sel], D[sel], I[sel], mn[sel], mx[sel])
            assert np.array_equal(occ, g["hit"]) and (occ[dropped] == 0).all(), "a dropped character casts no shadow"
            g = eng.scene_intersect(O, D, whole, mn, mx)
            assert not np.isin(g["instance"], np.flatnonzero(~kept)).any(), what
            _same_bytes(g, _expected_whole(ctx, only, O, D, mn, mx)[0], what)
            assert np.array_equal(eng.scene_occluded(O, D, whole, mn, mx), g["hit"])
        # a skin stage that no refit follows: nobody has a record
        eng.reserve_vertices(0)
        eng.set_mesh_variants(_patterns()["blocks"])
        ctx.tick(refit=False)
        _, rec = eng.blas_variant_bounds()
        assert (rec == A.NO_VARIANT).all()
        assert eng.scene_crowd_status().crowdReady == 1 and eng.scene_crowd_status().ragged == 1 and eng.scene_info().crowdReady == 1
        g = eng.scene_intersect(O, D, whole, mn, mx)
        _same_bytes(g, statics_only, "no record: the statics' answers, unchanged")
        assert np.array_equal(eng.scene_occluded(O, D, whole, mn, mx), statics_only["hit"])
        sel = I >= 0
        assert (eng.scene_intersect(O[sel], D[sel], I[sel], mn[sel], mx[sel])["hit"] == 0).all()
        assert (eng.scene_occluded(O[sel], D[sel], I[sel], mn[sel], mx[sel]) == 0).all()
        # the next refit brings the crowd back, as the launch that ran skinned it
        eng.blas_refit()
        g = eng.scene_intersect(O, D, whole, mn, mx)
        _same_bytes(g, _expected_whole(ctx, only, O, D, mn, mx)[0], "after the refit")
        assert ((g["instance"] >= 0) & (g["instance"] < CHARS)).any()
        # the live bytes change, the records do not: no answer changes
        eng.lod_select((0.0, 0.0, 0.0), [1.0])
        _same_bytes(eng.scene_intersect(O, D, whole, mn, mx), g, "after a later sge_lod_select")
        assert np.array_equal(eng.scene_occluded(O, D, whole, mn, mx), g["hit"])
    finally:
        eng.reserve_vertices(0)


def test_contract(sge):
    A = sge.abi

    def status(eng):
        st, info = eng.scene_crowd_status(), eng.scene_info()
        assert st.crowdReady == info.crowdReady and (st.reason == A.SCENE_CROWD_OK) == (st.crowdReady == 1)
        return (st.crowdReady, st.ragged, st.reason, st.variant)

    ctx = _Ctx(sge, "packed", range(NV), build=False)
    try:
        eng = ctx.eng
        assert status(eng) == (0, 0, A.SCENE_CROWD_NO_STRUCTURE, -1)
        eng.blas_build(_mesh(0)["indices"])
        assert status(eng) == (0, 0, A.SCENE_CROWD_VARIANT_NOT_BUILT, 1)
        for v in (3, 1):
            eng.blas_variant_build(v, _mesh(v)["indices"])
        assert status(eng) == (0, 0, A.SCENE_CROWD_VARIANT_NOT_BUILT, 2)
        eng.blas_variant_build(2, _mesh(2)["indices"])
        assert status(eng) == (1, 1, A.SCENE_CROWD_OK, -1)
        eng.upload_mesh_variant(3, _mesh(3))
        assert status(eng) == (0, 0, A.SCENE_CROWD_VARIANT_NOT_BUILT, 3)
        eng.blas_variant_build(3, _mesh(3)["indices"])
        assert status(eng) == (1, 1, A.SCENE_CROWD_OK, -1)
    finally:
        ctx.eng.close()
    uni = _Ctx(sge, "packed", [1])
    try:
        assert status(uni.eng) == (1, 0, A.SCENE_CROWD_OK, -1)
    finally:
        uni.eng.close()
    bare = sge.CharacterEngine(0)
    try:
        assert status(bare) == (0, 0, A.SCENE_CROWD_NO_MESH, -1)
    finally:
        bare.close()


def _look_at(eye, target, fov_y, aspect):
    """inverse(projection * view) as a row-major float64 4x4 (right-handed, -z forward)."""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    f = target - eye; f /= np.linalg.norm(f)
    s = np.cross(f, (0.0, 1.0, 0.0)); s /= np.linalg.norm(s)
    u = np.cross(s, f)
    view = np.eye(4); view[0, :3], view[1, :3], view[2, :3] = s, u, -f
    view[:3, 3] = -view[:3, :3] @ eye
    t = 1.0 / np.tan(fov_y / 2)
    near, far = 0.1, 5000.0
    proj = np.array([[t / aspect, 0, 0, 0], [0, t, 0, 0], [0, 0, far / (near - far), near * far / (near - far)], [0, 0, -1, 0]])
    return np.linalg.inv(proj @ view)


def test_six_ticks_under_every_overlap_mode_give_the_same_queries_and_frames(sge):
    """Overlap 0, 1 and 2 on a caller's stream, no host synchronisation in the loop: behind every tick the closest-hit, the any-hit
    and the frame launch are enqueued into buffers of their own. The outputs are byte-identical across the three modes."""
    import torch
    A = sge.abi
    rng = np.random.default_rng(3)
    assigns = [rng.integers(0, NV, CHARS) for _ in range(TICKS)]
    st = A.STAGE_ALL | A.STAGE_BLAS_REFIT
    W, H = 24, 16
    outs = []
    rays = frame = None
    for overlap in (0, 1, 2):
        eng = _scene_ctx(sge, overlap, list(range(NV)))
        lib, h = eng.t.lib, eng.h
        try:
            if rays is None:  # aimed at where a serial first tick leaves the characters
                eng.set_mesh_variants(assigns[0])
                eng.tick(dt=0.0, stages=A.STAGE_SKIN | A.STAGE_BLAS_REFIT)
                off = eng.vertex_offsets()
                pos = eng.skinned(0, int(off[-1]))[0]
                tgt = np.stack([pos[off[c]:off[c + 1]].mean(0) for c in range(CHARS)])
                lo, hi = pos.min(0), pos.max(0)
                d = np.tile(DIRS, (CHARS // 3 + 1, 1))[:CHARS]
                rays = eng._scene_rays(tgt - d * FAR, d, -1, 0.001, 1e6)
                eye = (lo + hi) / 2 + np.array([0.3, 0.4, 1.0]) * (np.linalg.norm(hi - lo) * 0.8 + 10)
                frame = sge.CharacterEngine.render_frame_record(_look_at(eye, (lo + hi) / 2, 0.9, W / H), eye, W, H, 1)
                ground = (lo - 30, hi + 30)
                eng.close()
                eng = _scene_ctx(sge, overlap, list(range(NV)))
                lib, h = eng.t.lib, eng.h
            (gx0, gy0, gz0), (gx1, _, gz1) = ground
            plane = _dress(np.array([[gx0, gy0, gz0], [gx1, gy0, gz0], [gx1, gy0, gz1], [gx0, gy0, gz1]], np.float32), [0, 2, 1, 0, 3, 2], 31)
            _set_statics(eng, {0: plane}, np.array([0], np.int32), np.eye(4, dtype=np.float32)[None])
            lights = np.zeros(1, A.render_light_dtype)
            lights["direction"], lights["intensity"], lights["color"], lights["enabled"], lights["maxDistance"] = (-0.3, -1.0, -0.2), 2.0, (1, 1, 1), 1.0, 1e5
            eng.render_lights(lights)
            dev = torch.device("cuda", 0)
            caller = torch.cuda.Stream(device=0)
            d_rays = torch.from_numpy(rays.view(np.uint8).copy()).to(dev)
            torch.cuda.synchronize()
            assert lib.sge_context_set_stream(h, C.c_void_p(caller.cuda_stream)) == 0
            bufs = []
            for a in assigns:
                eng.set_mesh_variants(a)
                eng.tick(stages=st)
                b = [torch.zeros(len(rays) * A.blas_hit_dtype.itemsize, dtype=torch.uint8, device=dev), torch.zeros(len(rays), dtype=torch.int32, device=dev),
                     torch.zeros(W * H * 4, dtype=torch.float32, device=dev), torch.zeros(W * H * A.render_aov_dtype.itemsize, dtype=torch.uint8, device=dev)]
                eng.scene_intersect_device(d_rays.data_ptr(), len(rays), b[0].data_ptr())
                eng.scene_occluded_device(d_rays.data_ptr(), len(rays), b[1].data_ptr())
                eng.render_frame_device(frame, b[2].data_ptr(), b[3].data_ptr())
                bufs.append(b)
            eng.synchronize()
            caller.synchronize()
            torch.cuda.synchronize()
            assert eng.scene_crowd_status().ragged == 1
            outs.append([[x.cpu().numpy() for x in b] for b in bufs])
            assert lib.sge_context_set_stream(h, None) == 0
        finally:
            eng.close()
    for t in range(TICKS):
        hits = outs[0][t][0].view(A.blas_hit_dtype)
        aov = outs[0][t][3].view(A.render_aov_dtype)
        assert np.array_equal(outs[0][t][1], hits["hit"])
        for mode in (1, 2):
            for k in range(4):
                assert np.array_equal(outs[0][t][k].view(np.uint8), outs[mode][t][k].view(np.uint8)), (mode, t, k)
    hits = outs[0][-1][0].view(A.blas_hit_dtype)
    aov = outs[0][-1][3].view(A.render_aov_dtype)
    assert ((hits["instance"] >= 0) & (hits["instance"] < CHARS)).any(), "the rays reach the crowd"
    assert ((aov["instance"] >= 0) & (aov["instance"] < CHARS)).any(), "the crowd is in the frame"


def test_a_frame_over_variants_that_hold_one_mesh_is_the_uniform_frame(sge):
    """All four variants hold mesh 1, variants 1..3 with 1, 64 and 1000 unreferenced vertices appended: the structures are identical,
    the vertex offsets are not. The frame under a mixed assignment is the frame of a uniform context over that mesh, byte for byte."""
    A = sge.abi
    base = _mesh(1)
    V = SHAPES[1][0]

    def padded(extra, seed):
        if extra == 0:
            return base
        more = _pad_case(base, extra, seed)
        assert more["indices"].max() < V and len(more["positions"]) == V + extra
        return more

    meshes = [padded(e, 90 + k) for k, e in enumerate((0, 1, 64, 1000))]
    W, H = 48, 32
    frames = []
    for variants in (meshes, meshes[:1]):
        eng = sge.CharacterEngine(0)
        try:
            eng.set_option(A.OPT_PLACEMENT_PROBES, 1)
            eng.set_option(A.OPT_FUSE_BLAS_REFIT, 0)
            rig = _rig()
            eng.upload_skeleton(rig)
            eng.upload_profiles(rig.profiles)
            eng.upload_skinned_mesh(variants[0])
            for k, m in enumerate(variants[1:], 1):
                eng.upload_mesh_variant(k, m)
            sge.crowd.spawn_crowd(eng, rig, CHARS, None, mode="lbs")
            eng.blas_build(variants[0]["indices"])
            eng.blas_set_uvs(variants[0]["uvs"])
            for k, m in enumerate(variants[1:], 1):
                eng.blas_variant_build(k, m["indices"])
                eng.blas_variant_set_uvs(k, m["uvs"])
            eng.blas_instances(_cols(_instances()))
            eng.synchronize()
            p = C.c_void_p()
            eng._call("crowd_buffers", C.byref(p), None, None, None)
            pal = np.ascontiguousarray(_palettes(), np.float32)
            assert _hip().hipMemcpy(p, pal.ctypes.data, pal.nbytes, 1) == 0
            if len(variants) > 1:
                eng.set_mesh_variants(_patterns()["mixed"])
            eng.tick(dt=0.0, stages=A.STAGE_SKIN | A.STAGE_BLAS_REFIT)
            st = eng.scene_crowd_status()
            assert (st.crowdReady, st.ragged) == (1, 1 if len(variants) > 1 else 0)
            lo = np.array([-300.0, -300.0, -300.0]); hi = np.array([35.0 * CHARS + 300, 300.0, 400.0])
            plane = _dress(np.array([[lo[0], lo[1], hi[2]], [hi[0], lo[1], hi[2]], [hi[0], hi[1], hi[2]], [lo[0], hi[1], hi[2]]], np.float32), [0, 1, 2, 0, 2, 3], 41)
            _set_statics(eng, {0: plane}, np.array([0], np.int32), np.eye(4, dtype=np.float32)[None])
            mats = A.default_render_materials(4)
            mats["alpha"][1], mats["metallic"][2], mats["roughness"][2], mats["transmission"][3], mats["alpha"][3] = 0.5, 1.0, 0.05, 0.7, 0.8
            eng.render_materials(mats)
            eng.render_crowd_materials(np.arange(CHARS) % 4)
            eng.render_static_materials([2])
            lights = np.zeros(2, A.render_light_dtype)
            lights["direction"], lights["intensity"], lights["color"], lights["enabled"], lights["maxDistance"] = [(-0.3, -0.5, 1.0), (0.4, -0.2, 0.8)], 2.0, (1, 1, 1), 1.0, 1e5
            eng.render_lights(lights)
            eye = np.array([35.0 * CHARS / 2, 30.0, -900.0])
            frame = sge.CharacterEngine.render_frame_record(_look_at(eye, (35.0 * CHARS / 2, 0.0, 40.0), 1.4, W / H), eye, W, H, 2)
            frames.append(eng.render_frame(frame, aov=True))
        finally:
            eng.close()
    (rgba, aov), (urgba, uaov) = frames
    assert ((aov["instance"] >= 0) & (aov["instance"] < CHARS)).sum() >= 8, "the crowd is in the frame"
    assert np.array_equal(rgba.view(np.uint32), urgba.view(np.uint32))
    for f in aov.dtype.names:
        assert np.array_equal(aov[f].view(np.uint32), uaov[f].view(np.uint32)), f


def _pad_case(case, extra, seed):
    """The mesh with `extra` vertices nobody references appended to every per-vertex array."""
    rng = np.random.default_rng(seed)
    V = len(case["positions"])
    out = {}
    for k, a in case.items():
        a = np.asarray(a)
        if k == "indices" or a.shape[0] != V:
            out[k] = a
            continue
        pick = rng.integers(0, V, extra)
        out[k] = np.ascontiguousarray(np.concatenate([a, a[pick]]))
    return out


def test_a_frame_over_different_variants_against_the_reference(sge):
    """The four genuinely different variants in the scene of tests/render_variant_scenes.py: a mirror wall that reflects characters, a
    translucent sheet and translucent characters in front of characters of other variants, a refractive character, two lights.
    Compared with RenderRef over SceneRef + VariantCrowdRef by the stable-pixel rule and the bar construction of
    tests/test_gpu_render.py (its _check): AOV fields exact on stable pixels, rgb within 4 x the scene's float32 restatement figure.
    Packed layout only: the reference scans every triangle of the crowd on the CPU per query, 15 to 30 s for this frame. Measured:
    2.99 % of the pixels unstable in the reference alone, restatement worst 3.593e-7, GPU worst |rgb - ref| 3.593e-7 = 0.25 of the bar."""
    import render_scenes as rs
    import render_variant_scenes as rv
    from render_ref import RenderRef
    from test_gpu_render import _check, _renders
    ctx = _Ctx(sge, "packed", range(NV))
    scene = crowd = None
    try:
        eng = ctx.eng
        ctx.write_palettes(_palettes())
        eng.blas_instances(_cols(rv.instances()))
        eng.set_mesh_variants(_patterns()["mixed"])
        ctx.tick()
        off = eng.vertex_offsets()
        p, n, t = eng.skinned(0, int(off[-1]))
        _, rec = eng.blas_variant_bounds()
        meshes, mesh_of, mats, material_of = rv.statics()
        rs.upload_scene(eng, meshes, mesh_of, mats)
        m, lights = rs.materials(sge), rv.lights(sge)
        eng.render_materials(m)
        eng.render_static_materials(material_of)
        eng.render_crowd_materials(rv.crowd_materials())
        eng.render_lights(lights)
        vm = [dict(_mesh(v), tangents=np.tile(np.array([1, 0, 0, 1], np.float32), (SHAPES[v][0], 1))) for v in range(NV)]
        crowd = VariantCrowdRef(sge, vm, rec, off, p, n, t, _cols(rv.instances()))
        scene = SceneRef(sge, meshes, mesh_of, mats, crowd=crowd)
        ref = RenderRef(scene, m, material_of, rv.crowd_materials(), lights)
        eye, target = rv.camera()
        f = rs.frame_record(sge, eye, target, rv.SIZE[0], rv.SIZE[1], 2)
        a, b, a32 = _renders(ref, f)
        seen = a["instance"][(a["instance"] >= 0) & (a["instance"] < CHARS)]
        assert len(set(rec[seen].tolist())) >= 3, "primary hits on characters of at least three variants"
        assert (a["flags"] & 1).any() and (a["flags"] & 2).any() and ((a["shadow"] > 0) & (a["shadow"] < 1)).any() and a["layers"].max() == 3
        rgba, aov = eng.render_frame(f, aov=True)
        old = rs.RESTATEMENT_WORST
        rs.RESTATEMENT_WORST = dict(old, **rv.RESTATEMENT_WORST)  # _check looks the scene's figure up by name
        try:
            _check("variant crowd packed", rgba, aov, a, b, a32, eng, f, np.asarray(eye, np.float32))
        finally:
            rs.RESTATEMENT_WORST = old
    finally:
        ctx.eng.close()
        if scene is not None:
            scene.close()
        if crowd is not None:
            crowd.close()
