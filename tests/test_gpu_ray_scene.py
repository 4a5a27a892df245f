"""GPU tests of the ray scene (include/sge_amd_ray_scene.h): static mesh instances beside the crowd, closest hit and occlusion.

Reference: scene_ref.SceneRef — the CPU oracle's scan over every triangle, one oracle engine per static mesh and one for the
crowd (fed the GPU's skinned streams), composed by the header's rule (distance bits, scene id, primitive id). Bars, those of
test_gpu_blas.py: hit / primitive / instance exact, floats within 1e-6 * max(1, |ref|.max()); the static meshes' boxes are
value-exact against blas_ref.expected_bounds; occlusion equals the composed record's `hit` exactly.
"""
import numpy as np
import pytest

import oracle_binding as ob
from blas_ref import expected_bounds
from scene_ref import STATIC_BASE, SceneRef, assert_records_match, columns
from scenes import build_scene

pytestmark = pytest.mark.gpu


# ---- meshes ---------------------------------------------------------------------------------------------------------------
def _dress(pos, idx, seed):
    """Random unit normals, tangents with w = +-1 and uvs for a vertex / index set."""
    rng = np.random.default_rng(seed)
    V = len(pos)
    n = rng.normal(size=(V, 3)); n /= np.linalg.norm(n, axis=1, keepdims=True)
    t = rng.normal(size=(V, 3)); t /= np.linalg.norm(t, axis=1, keepdims=True)
    tan = np.concatenate([t, rng.choice([-1.0, 1.0], (V, 1))], 1)
    return {"positions": np.ascontiguousarray(pos, np.float32), "normals": n.astype(np.float32), "tangents": tan.astype(np.float32),
            "uvs": rng.uniform(0, 1, (V, 2)).astype(np.float32), "indices": np.ascontiguousarray(idx, np.uint32).reshape(-1)}


def _one_triangle():
    return _dress(np.array([[-0.4, -0.4, 0], [0.4, -0.4, 0], [0, 0.4, 0]], np.float32), [0, 1, 2], 1)


def _ribbon(t):
    """t separate triangles along a bent ribbon."""
    i = np.arange(t, dtype=np.float32)
    a = np.stack([i * 0.25, np.zeros(t), np.sin(i * 0.3)], 1)
    c = a + np.stack([np.full(t, 0.12), np.full(t, 0.5), 0.1 * np.cos(i)], 1)
    pos = np.stack([a, a + (0.3, 0, 0.05), c], 1).reshape(-1, 3)
    return _dress(pos, np.arange(3 * t), 2 + t)


def _grid(q=46):
    """q x q quads (2 q^2 triangles) over [0, 4]^2 with a height field."""
    u = np.linspace(0, 4, q + 1, dtype=np.float32)
    X, Z = np.meshgrid(u, u, indexing="ij")
    pos = np.stack([X, 0.3 * np.sin(2 * X) * np.cos(1.5 * Z), Z], -1).reshape(-1, 3)
    v = np.arange((q + 1) * (q + 1)).reshape(q + 1, q + 1)
    a, b, c, d = v[:-1, :-1].ravel(), v[1:, :-1].ravel(), v[1:, 1:].ravel(), v[:-1, 1:].ravel()
    return _dress(pos, np.stack([a, d, b, b, d, c], 1).reshape(-1), 7)


def _mirror(sge):
    z = np.load(sge.assets.GOLDEN_DIR + "/ornate_mirror_static.npz")
    return _dress(z["positions"], z["indices"], 9)


def _upload(gpu, mesh_id, m):
    return gpu.scene_mesh_upload(mesh_id, m["positions"], m["normals"], m["tangents"], m["indices"], uvs=m.get("uvs"))


def _rotation(axis, angle):
    a = np.asarray(axis, np.float64); a /= np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return (np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K).astype(np.float32)


def _four_matrices():
    """identity, translation, rotation + translation, non-uniform scale with a negative determinant"""
    mats = np.tile(np.eye(4, dtype=np.float32), (4, 1, 1))
    mats[1][:3, 3] = (7, -2, 3)
    mats[2][:3, :3] = _rotation((0.3, 0.8, -0.5), 1.1)
    mats[2][:3, 3] = (-6, 1, 9)
    mats[3][:3, :3] = np.diag([1.5, -0.75, 2.0]) @ np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], np.float32)
    mats[3][:3, 3] = (1, 8, -7)
    assert np.linalg.det(mats[3][:3, :3]) < 0
    return mats


def _rays_at(rng, lo, hi, k):
    """k rays from a shell around the box [lo, hi] towards random points inside it (test_gpu_blas.py)."""
    centre, half = (lo + hi) / 2, (hi - lo) / 2
    d = rng.normal(size=(k, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    origins = centre + d * (np.linalg.norm(half) * rng.uniform(1.2, 3.0, (k, 1)))
    targets = centre + rng.uniform(-1, 1, (k, 3)) * half
    dirs = targets - origins
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    return origins.astype(np.float32), dirs.astype(np.float32)


def _static_rays(meshes, mesh_of, mats, seed=11, per=600):
    """Aimed rays per instance, rays through vertices and edge midpoints, axis-parallel rays, rays starting between instances.
    -> origins, directions, the scene id each ray was built for"""
    rng = np.random.default_rng(seed)
    O, D, I = [], [], []
    centres = []
    for s, m in enumerate(mesh_of):
        mesh = meshes[m]
        world = mesh["positions"] @ mats[s][:3, :3].T + mats[s][:3, 3]
        centres.append(world.mean(0))
        o, d = _rays_at(rng, world.min(0), world.max(0), per)
        O.append(o); D.append(d); I.append(np.full(len(o), STATIC_BASE + s, np.int32))
        tri = mesh["indices"].reshape(-1, 3)[rng.integers(0, len(mesh["indices"]) // 3, 60)]
        tgt = np.concatenate([world[tri[:30, 0]], (world[tri[30:, 0]] + world[tri[30:, 1]]) / 2]).astype(np.float32)
        o2 = (tgt + rng.normal(size=(60, 3)) * 0.01 + np.array([0.3, 4.0, 0.2]) @ mats[s][:3, :3].T).astype(np.float32)
        d2 = tgt - o2
        O.append(o2); D.append((d2 / np.linalg.norm(d2, axis=1, keepdims=True)).astype(np.float32)); I.append(np.full(60, STATIC_BASE + s, np.int32))
        # axis-parallel (zero direction components), straight down onto the instance
        o3 = (world[rng.integers(0, len(world), 8)] + (0, 5, 0)).astype(np.float32)
        O.append(o3); D.append(np.tile(np.array([0, -1, 0], np.float32), (8, 1))); I.append(np.full(8, STATIC_BASE + s, np.int32))
    centres = np.array(centres)
    for a in range(len(centres)):  # from between two instances towards each of them
        b = (a + 1) % len(centres)
        mid = ((centres[a] + centres[b]) / 2).astype(np.float32)
        for tgt, s in ((centres[a], a), (centres[b], b)):
            d = tgt - mid
            if np.linalg.norm(d) > 1e-3:
                O.append(mid[None]); D.append((d / np.linalg.norm(d)).astype(np.float32)[None]); I.append(np.array([STATIC_BASE + s], np.int32))
    return np.concatenate(O).astype(np.float32), np.concatenate(D).astype(np.float32), np.concatenate(I)


def _device_query(sge, gpu, O, D, inst, occluded=False, min_distance=0.001, max_distance=1e6):
    import torch
    r = np.zeros(len(O), sge.abi.blas_ray_dtype)
    r["origin"], r["direction"], r["minDistance"], r["maxDistance"], r["instance"] = O, D, min_distance, max_distance, inst
    d_r = torch.from_numpy(r.view(np.uint8).copy()).to("cuda:0")
    size = 4 if occluded else sge.abi.blas_hit_dtype.itemsize
    d_o = torch.zeros(len(O) * size, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    (gpu.scene_occluded_device if occluded else gpu.scene_intersect_device)(d_r.data_ptr(), len(O), d_o.data_ptr())
    gpu.synchronize()
    return d_o.cpu().numpy().view(np.int32 if occluded else sge.abi.blas_hit_dtype)


# ---- 1. static boxes ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["1", "64", "65", "grid46", "mirror"])
def test_static_mesh_boxes_are_exact(sge, shape):
    mesh = {"1": _one_triangle, "64": lambda: _ribbon(64), "65": lambda: _ribbon(65), "grid46": _grid, "mirror": lambda: _mirror(sge)}[shape]()
    gpu = sge.CharacterEngine(0)
    try:
        info = _upload(gpu, 3, mesh)
        topo = sge.CharacterEngine.blas_topology(mesh["positions"], mesh["indices"])
        assert (info.triangleCount, info.entryCount, info.wideCount, info.clusterCount) == \
               (len(mesh["indices"]) // 3, topo["info"].entryCount, topo["info"].wideCount, topo["info"].clusterCount)
        if shape in ("1", "64"):
            assert info.clusterCount == 1
        if shape == "65":
            assert info.clusterCount == 2
        if shape == "grid46":
            assert info.triangleCount == 4232 and info.clusterCount > 64 and info.wideCount > 1
        got = gpu.scene_mesh_bounds(3)
        want = expected_bounds(topo, mesh["indices"], mesh["positions"])
        assert got.shape == want.shape and np.array_equal(got, want), np.argwhere(got != want)[:4]
        assert gpu.scene_info().meshes == 1
    finally:
        gpu.close()


# ---- 2. + 5. statics alone ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def statics_case(sge):
    """Four instances (65-triangle ribbon, grid, ribbon, grid), no crowd in the context; rays, reference records and the GPU's,
    computed once and shared."""
    meshes = {0: _ribbon(65), 5: _grid()}
    mesh_of = [0, 5, 0, 5]
    mats = _four_matrices()
    gpu = sge.CharacterEngine(0)
    ref = SceneRef(sge, meshes, mesh_of, mats)
    try:
        for m, mesh in meshes.items():
            _upload(gpu, m, mesh)
        gpu.scene_instances(mesh_of, columns(mats))
        O, D, I = _static_rays(meshes, mesh_of, mats)
        A = np.full(len(O), -1, np.int32)
        yield {"gpu": gpu, "ref": ref, "O": O, "D": D, "I": I, "A": A, "meshes": meshes, "mesh_of": mesh_of, "mats": mats,
               "named": (gpu.scene_intersect(O, D, I), ref.intersect(O, D, I)), "whole": (gpu.scene_intersect(O, D, A), ref.intersect(O, D, A))}
    finally:
        gpu.close(); ref.close()


def test_statics_alone_match_the_triangle_scan(sge, statics_case):
    c = statics_case
    gpu, ref, O, D, I, A = c["gpu"], c["ref"], c["O"], c["D"], c["I"], c["A"]
    info = gpu.scene_info()
    assert (info.meshes, info.staticInstances, info.characters, info.crowdReady) == (2, 4, 0, 0)
    for what in ("named", "whole"):
        g, w = c[what]
        assert w["hit"].sum() >= 0.2 * len(O) and (w["hit"] == 0).any(), (what, w["hit"].mean())
        assert_records_match(g, w, what)
        assert np.abs(g["uv"][g["hit"] == 1]).max() > 0.1
    g, w = c["named"]
    assert np.array_equal(g["instance"], np.where(g["hit"] == 1, I, -1))
    ga = c["whole"][0]
    assert set(np.unique(ga["instance"][ga["hit"] == 1]).tolist()) == {STATIC_BASE + s for s in range(4)}, "every instance is hit by some whole-scene ray"
    # distance limits, as in test_closest_hit_matches_the_triangle_scan
    lim = np.where(g["hit"] == 1, g["distance"] * 0.5, 1.0).astype(np.float32)
    for inst in (I, A):
        assert_records_match(gpu.scene_intersect(O, D, inst, max_distance=lim), ref.intersect(O, D, inst, max_distance=lim), "max_distance")
        g2, w2 = gpu.scene_intersect(O, D, inst, min_distance=lim), ref.intersect(O, D, inst, min_distance=lim)
        assert_records_match(g2, w2, "min_distance")
        assert (g2["distance"][g2["hit"] == 1] >= lim[g2["hit"] == 1]).all()
    # ids that name nothing: a static instance beyond the list, a character (there is no crowd), the largest id
    miss = gpu.scene_intersect(O[:3], D[:3], [STATIC_BASE + 4, 0, 0x7fffffff])
    assert miss["hit"].tolist() == [0, 0, 0] and miss["instance"].tolist() == [-1, -1, -1]
    # the device entry point gives the same records
    hd = _device_query(sge, gpu, O, D, A)
    for f in hd.dtype.names:
        assert np.array_equal(hd[f], ga[f]), f


def test_two_statics_at_the_same_place_the_smaller_id_wins(sge, statics_case):
    c = statics_case
    gpu, ref = c["gpu"], c["ref"]
    mats = c["mats"].copy()
    mats[2] = mats[0]  # instances 0 and 2 are both the ribbon
    try:
        gpu.scene_instances_update(columns(mats))
        ref.set_matrices(mats)
        sel = (c["I"] == STATIC_BASE) | (c["I"] == STATIC_BASE + 2)
        O, D = c["O"][sel], c["D"][sel]
        g, w = gpu.scene_intersect(O, D, -1), ref.intersect(O, D, -1)
        assert_records_match(g, w, "twins")
        assert (g["instance"] == STATIC_BASE).sum() > 100 and not (g["instance"] == STATIC_BASE + 2).any()
    finally:
        gpu.scene_instances_update(columns(c["mats"]))
        ref.set_matrices(c["mats"])


def test_occlusion_of_statics_equals_the_composed_hit(sge, statics_case):
    c = statics_case
    gpu, ref, O, D, I, A = c["gpu"], c["ref"], c["O"], c["D"], c["I"], c["A"]
    for inst, what in ((I, "named"), (A, "whole")):
        occ = gpu.scene_occluded(O, D, inst)
        assert np.array_equal(occ, c[what][1]["hit"]), np.argwhere(occ != c[what][1]["hit"])[:5].ravel()
        assert (occ == 1).any() and (occ == 0).any()
    # a blocker beyond maxDistance or before minDistance does not occlude
    w = c["whole"][1]
    hit = w["hit"] == 1
    near = np.where(hit, w["distance"] * 0.5, 1.0).astype(np.float32)
    far = np.where(hit, w["distance"] * 1.5 + 0.01, 1.0).astype(np.float32)
    o_near = gpu.scene_occluded(O, D, A, max_distance=near)
    assert np.array_equal(o_near, ref.intersect(O, D, A, max_distance=near)["hit"]) and (o_near[hit] == 0).sum() > 100
    o_far = gpu.scene_occluded(O, D, A, min_distance=far)
    w_far = ref.intersect(O, D, A, min_distance=far)
    print("beyond the first hit: occluded %d, reference %d, differing %s" % (o_far.sum(), w_far["hit"].sum(), np.flatnonzero(o_far != w_far["hit"])[:8]))
    assert_records_match(gpu.scene_intersect(O, D, A, min_distance=far), w_far, "beyond the first hit")
    assert np.array_equal(o_far, w_far["hit"]) and (o_far[hit] == 0).sum() > 100
    # the device entry point gives the same words
    assert np.array_equal(_device_query(sge, gpu, O, D, A, occluded=True), gpu.scene_occluded(O, D, A))
    assert np.array_equal(_device_query(sge, gpu, O, D, I, occluded=True, max_distance=2.0), gpu.scene_occluded(O, D, I, max_distance=2.0))


# ---- 3. instance-level boundaries --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [1, 64, 65, 4097])
def test_instance_level_boundaries(sge, count):
    """65 instances: a second group of 64; 4,097: a second step of the scan over group boxes."""
    tri = _one_triangle()
    side = int(np.ceil(np.sqrt(count)))
    k = np.arange(count)
    mats = np.tile(np.eye(4, dtype=np.float32), (count, 1, 1))
    mats[:, 0, 3], mats[:, 1, 3] = (k % side) * 2.0, (k // side) * 2.0   # a lattice in the XY plane, triangles facing +-Z
    gpu = sge.CharacterEngine(0)
    ref = SceneRef(sge, {0: tri}, np.zeros(count, np.int32), mats)
    try:
        _upload(gpu, 0, tri)
        gpu.scene_instances(np.zeros(count, np.int32), columns(mats))
        assert gpu.scene_info().staticInstances == count
        # one ray per instance at its centre
        O = (mats[:, :3, 3] + (0, -0.1, -3)).astype(np.float32)
        D = np.tile(np.array([0, 0, 1], np.float32), (count, 1))
        g, w = gpu.scene_intersect(O, D, -1), ref.intersect(O, D, -1)
        assert_records_match(g, w, "centres")
        assert np.array_equal(g["instance"], STATIC_BASE + k) and (g["hit"] == 1).all()
        named = gpu.scene_intersect(O, D, STATIC_BASE + k)
        for f in named.dtype.names:
            assert np.array_equal(named[f], g[f]), f
        assert np.array_equal(gpu.scene_occluded(O, D, -1), np.ones(count, np.int32))
        # along every lattice row, in the triangles' plane is a miss; tilted through the row from either end: the nearest is reported
        rows = (count + side - 1) // side
        y = (np.arange(rows) * 2.0 - 0.1).astype(np.float32)
        O2 = np.concatenate([np.stack([np.full(rows, -3.0), y, np.full(rows, -0.05)], 1), np.stack([np.full(rows, side * 2.0 + 1), y, np.full(rows, 0.05)], 1)]).astype(np.float32)
        D2 = np.concatenate([np.tile([1.0, 0, 0.016], (rows, 1)), np.tile([-1.0, 0, -0.016], (rows, 1))]).astype(np.float32)
        D2 /= np.linalg.norm(D2, axis=1, keepdims=True)
        g2, w2 = gpu.scene_intersect(O2, D2, -1), ref.intersect(O2, D2, -1)
        assert_records_match(g2, w2, "rows")
        assert g2["hit"].sum() >= rows
        assert np.array_equal(gpu.scene_occluded(O2, D2, -1), w2["hit"])
    finally:
        gpu.close(); ref.close()


# ---- 4. + 5. crowd + statics ----------------------------------------------------------------------------------------------------
def _crowd(sge, layout, n=3):
    gpu, cpu = sge.CharacterEngine(0), ob.oracle_engine()
    gpu.set_option(sge.abi.OPT_SKIN_LAYOUT, sge.abi.LAYOUT_PADDED16 if layout == "padded16" else sge.abi.LAYOUT_PACKED)
    for e in (gpu, cpu):
        build_scene(sge, e, n, terrain_cells=(24, 16), rings=9, segments=8, mixed=True, seed=5)
        e.blas_build(e.mesh["indices"])
    uvs = np.random.default_rng(2).uniform(0, 1, (gpu.vertex_count, 2)).astype(np.float32)
    for e in (gpu, cpu):
        e.blas_set_uvs(uvs)
    for _ in range(4):
        gpu.tick(stages=sge.abi.STAGE_ALL | sge.abi.STAGE_BLAS_REFIT)
    gp, gn, gt = gpu.skinned()
    ob.skinned_upload(cpu, gp, gn, gt)  # both sides look at the same skinned vertices
    return gpu, cpu, gp


@pytest.mark.parametrize("layout", ["packed", "padded16"])
def test_crowd_and_statics(sge, layout):
    gpu, cpu, gp = _crowd(sge, layout)
    ref = None
    try:
        n, V = 3, gpu.vertex_count
        chars = gp.reshape(n, V, 3)
        lo, hi = gp.min(0), gp.max(0)
        # a ground quad under the characters, a grid-mesh wall in front of character 0 (towards -z), and a 1-triangle mesh laid
        # exactly on triangle 0 of character 1 (same three float32 vertices, identity matrix)
        ground = _dress(np.array([[lo[0] - 5, lo[1] - 0.05, lo[2] - 5], [hi[0] + 5, lo[1] - 0.05, lo[2] - 5], [hi[0] + 5, lo[1] - 0.05, hi[2] + 5],
                                  [lo[0] - 5, lo[1] - 0.05, hi[2] + 5]], np.float32), [0, 2, 1, 0, 3, 2], 21)
        wall = _grid()
        t0 = gpu.mesh["indices"].reshape(-1, 3)[0]
        decal = _dress(chars[1][t0], [0, 1, 2], 22)
        meshes = {0: ground, 1: wall, 2: decal}
        mesh_of = [0, 1, 2]
        mats = np.tile(np.eye(4, dtype=np.float32), (3, 1, 1))
        c0 = chars[0].mean(0)
        ext = chars[0].max(0) - chars[0].min(0)
        sc = np.float32(1.2 * max(ext[0], ext[1]) / 4)  # the 4 x 4 grid, scaled to cover the character and stood up: its z becomes height
        mats[1][:3, :3] = sc * np.array([[1, 0, 0], [0, 0, 1], [0, -1, 0]], np.float32)
        mats[1][:3, 3] = (c0[0] - 2 * sc, c0[1] - 2 * sc, chars[0][:, 2].min() - 0.5 * ext[2] - 0.3 * sc)
        for m, mesh in meshes.items():
            _upload(gpu, m, mesh)
        gpu.scene_instances(mesh_of, columns(mats))
        info = gpu.scene_info()
        assert (info.meshes, info.staticInstances, info.characters, info.crowdReady) == (3, 3, n, 1)
        ref = SceneRef(sge, meshes, mesh_of, mats, crowd=cpu)
        rng = np.random.default_rng(4)
        O, D = [], []
        for c in range(n):
            o, d = _rays_at(rng, chars[c].min(0), chars[c].max(0), 500)
            O.append(o); D.append(d)
        o, d = _rays_at(rng, lo - (5, 1, 5), hi + (5, 0, 5), 400)
        O.append(o); D.append(d)
        # through the wall towards character 0
        tgt = chars[0][rng.integers(0, V, 100)]
        o = (tgt + (0, 0, -(3 * ext[2] + sc)) + rng.normal(size=(100, 3)) * 0.05 * ext).astype(np.float32)
        O.append(o); D.append(((tgt - o) / np.linalg.norm(tgt - o, axis=1, keepdims=True)).astype(np.float32))
        # at the decal / triangle 0 of character 1 from both sides
        ctr = chars[1][t0].mean(0)
        nrm = np.cross(chars[1][t0][1] - chars[1][t0][0], chars[1][t0][2] - chars[1][t0][0]); nrm /= np.linalg.norm(nrm)
        tie_o = np.array([ctr + nrm * 0.02, ctr + nrm * 0.05], np.float32)
        O.append(tie_o); D.append(np.tile(-nrm.astype(np.float32), (2, 1)))
        O, D = np.concatenate(O).astype(np.float32), np.concatenate(D).astype(np.float32)
        A = np.full(len(O), -1, np.int32)
        g, w = gpu.scene_intersect(O, D, A), ref.intersect(O, D, A)
        assert w["hit"].sum() >= 0.2 * len(O) and (w["hit"] == 0).any()
        assert_records_match(g, w, "whole scene")
        hit_ids = set(np.unique(g["instance"][g["hit"] == 1]).tolist())
        assert {0, 1, 2, STATIC_BASE, STATIC_BASE + 1} <= hit_ids, hit_ids
        # the tie: the static triangle lies exactly on the character's; the character (smaller scene id) is reported
        tie = g[-2:]
        assert (tie["hit"] == 1).all() and (tie["instance"] == 1).all() and (tie["primitive"] == 0).all(), tie[["instance", "primitive", "distance"]]
        alone = gpu.scene_intersect(tie_o, np.tile(-nrm.astype(np.float32), (2, 1)), STATIC_BASE + 2)
        assert np.array_equal(alone["distance"].view(np.uint32), tie["distance"].view(np.uint32)), "the two report the same distance bits"
        # a ray whose max_distance ends before the character behind the wall stops at the wall; one that passes the wall by
        # min_distance reaches the character
        thru = slice(len(O) - 102, len(O) - 2)
        first = g[thru]
        behind = first["instance"] == STATIC_BASE + 1
        assert behind.sum() > 20, "the wall stands in front of character 0"
        past = (first["distance"] + 0.01).astype(np.float32)
        g3, w3 = gpu.scene_intersect(O[thru], D[thru], -1, min_distance=past), ref.intersect(O[thru], D[thru], -1, min_distance=past)
        assert_records_match(g3, w3, "past the wall")
        assert (g3["instance"][behind] == 0).sum() > 10, "rays that pass the wall reach the character behind it"
        # named rays: characters and statics
        named = np.where(g["hit"] == 1, g["instance"], 0).astype(np.int32)
        assert_records_match(gpu.scene_intersect(O, D, named), ref.intersect(O, D, named), "named")
        # occlusion on these rays
        occ = gpu.scene_occluded(O, D, A)
        assert np.array_equal(occ, w["hit"]) and (occ == 1).any() and (occ == 0).any()
        lim = np.where(w["hit"] == 1, w["distance"] * 0.5, 1.0).astype(np.float32)
        assert np.array_equal(gpu.scene_occluded(O, D, A, max_distance=lim), ref.intersect(O, D, A, max_distance=lim)["hit"])
        assert np.array_equal(gpu.scene_occluded(O, D, named), ref.intersect(O, D, named)["hit"])
        assert np.array_equal(_device_query(sge, gpu, O, D, A, occluded=True), occ)
        # equality with the existing path: with the static list cleared the records are byte-identical to sge_blas_intersect_*
        gpu.scene_instances([], np.zeros((0, 16), np.float32))
        assert gpu.scene_info().staticInstances == 0
        chars_only = np.where((named >= 0) & (named < n), named, 1).astype(np.int32)
        for inst in (A, chars_only):
            a, b = gpu.scene_intersect(O, D, inst), gpu.blas_intersect(O, D, inst)
            assert a.tobytes() == b.tobytes()
            assert a["hit"].sum() > 100
        import torch
        for inst in (A, chars_only):  # the device entry points: whole-scene and named rays
            r = np.zeros(len(O), sge.abi.blas_ray_dtype)
            r["origin"], r["direction"], r["minDistance"], r["maxDistance"], r["instance"] = O, D, 0.001, 1e6, inst
            d_r = torch.from_numpy(r.view(np.uint8).copy()).to("cuda:0")
            d_h = torch.zeros(len(O) * sge.abi.blas_hit_dtype.itemsize, dtype=torch.uint8, device="cuda:0")
            torch.cuda.synchronize()
            gpu.blas_intersect_device(d_r.data_ptr(), len(O), d_h.data_ptr())
            gpu.synchronize()
            assert d_h.cpu().numpy().tobytes() == _device_query(sge, gpu, O, D, inst).tobytes()
    finally:
        gpu.close(); cpu.close()
        if ref is not None:
            ref.close()


# ---- 6. moving instances -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("overlap", [0, 1, 2])
def test_moving_instances_are_ordered_on_the_stream(sge, overlap):
    """sge_scene_instances_update, then device queries, nothing synchronised in between, behind ticks with skin + refit."""
    import torch
    gpu, cpu, gp = _crowd(sge, "packed")
    ref = None
    try:
        gpu.set_option(sge.abi.OPT_OVERLAP_SKIN, overlap)
        platform, ground = _ribbon(65), _grid()
        meshes, mesh_of = {0: platform, 1: ground}, [0, 1, 0]
        mats = np.tile(np.eye(4, dtype=np.float32), (3, 1, 1))
        # high above the crowd, and every ray ends after 200 units: no ray reaches a character, so the reference needs no crowd
        mats[0][:3, 3] = (30, 500, 0); mats[1][:3, 3] = (30, 510, 0); mats[2][:3, 3] = (30, 520, 0)
        for m, mesh in meshes.items():
            _upload(gpu, m, mesh)
        gpu.scene_instances(mesh_of, columns(mats))
        ref = SceneRef(sge, meshes, mesh_of, mats, crowd=None)
        rng = np.random.default_rng(6)
        world = [meshes[m]["positions"] @ mats[s][:3, :3].T + mats[s][:3, 3] for s, m in enumerate(mesh_of)]
        moved = mats.copy()
        moved[2][:3, :3] = _rotation((0, 0, 1), 0.4)
        moved[2][:3, 3] = (30, 540, 5)
        new_world = meshes[0]["positions"] @ moved[2][:3, :3].T + moved[2][:3, 3]
        O, D = zip(*[_rays_at(rng, w.min(0), w.max(0), 200) for w in world + [new_world]])
        O, D = np.concatenate(O), np.concatenate(D)
        before = gpu.scene_intersect(O, D, -1, max_distance=200.0)
        assert_records_match(before, ref.intersect(O, D, -1, max_distance=200.0), "before")
        r = np.zeros(len(O), sge.abi.blas_ray_dtype)
        r["origin"], r["direction"], r["minDistance"], r["maxDistance"], r["instance"] = O, D, 0.001, 200.0, -1
        d_r = torch.from_numpy(r.view(np.uint8).copy()).to("cuda:0")
        d_h = torch.zeros(len(O) * sge.abi.blas_hit_dtype.itemsize, dtype=torch.uint8, device="cuda:0")
        d_o = torch.zeros(len(O), dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        gpu.tick(stages=sge.abi.STAGE_ALL | sge.abi.STAGE_BLAS_REFIT)
        m = columns(moved[2:3]).copy()
        gpu.scene_instances_update(m, first=2)
        m[:] = np.nan  # the host array may be reused on return
        gpu.scene_intersect_device(d_r.data_ptr(), len(O), d_h.data_ptr())
        gpu.scene_occluded_device(d_r.data_ptr(), len(O), d_o.data_ptr())
        gpu.synchronize()
        after = d_h.cpu().numpy().view(sge.abi.blas_hit_dtype)
        ref.set_matrices(moved)
        want = ref.intersect(O, D, -1, max_distance=200.0)
        assert_records_match(after, want, "after")
        assert np.array_equal(d_o.cpu().numpy(), want["hit"])
        old, new = slice(400, 600), slice(600, 800)
        # (the records themselves are pinned above; these say that both outcomes occur: the ribbon is sparse, a handful of the
        # 200 rays aimed at its box hit it)
        was = before["instance"][old] == STATIC_BASE + 2
        assert was.sum() >= 5 and (after["instance"][old] != STATIC_BASE + 2).all(), "rays that hit at the old place no longer do"
        assert (after["instance"][new] == STATIC_BASE + 2).sum() >= 5 and (before["instance"][new] != STATIC_BASE + 2).all(), "rays at the new place hit"
        assert after[:400].tobytes() == before[:400].tobytes(), "the other instances' records are unchanged"
    finally:
        gpu.close(); cpu.close()
        if ref is not None:
            ref.close()


# ---- 7. contract ---------------------------------------------------------------------------------------------------------------
def test_contract(sge):
    gpu = sge.CharacterEngine(0)
    ref = None
    try:
        tri, rib = _one_triangle(), _ribbon(65)
        assert tuple(getattr(gpu.scene_info(), f) for f in ("meshes", "staticInstances", "characters", "crowdReady")) == (0, 0, 0, 0)
        # an empty scene answers: everything misses; count == 0 works
        assert gpu.scene_intersect([[0, 0, -3]], [[0, 0, 1]], -1)["hit"].tolist() == [0]
        assert gpu.scene_occluded([[0, 0, -3]], [[0, 0, 1]], -1).tolist() == [0]
        assert len(gpu.scene_intersect(np.zeros((0, 3)), np.zeros((0, 3)), -1)) == 0 and len(gpu.scene_occluded(np.zeros((0, 3)), np.zeros((0, 3)), -1)) == 0
        gpu.scene_intersect_device(0, 0, 0); gpu.scene_occluded_device(0, 0, 0)
        # sge_scene_mesh_upload fails as sge_blas_build fails
        with pytest.raises(sge.SgeError, match="bad argument"):
            gpu.scene_mesh_upload(0, tri["positions"], tri["normals"], tri["tangents"], np.zeros(0, np.uint32))
        with pytest.raises(sge.SgeError, match="out of range"):
            gpu.scene_mesh_upload(0, tri["positions"], tri["normals"], tri["tangents"], np.array([0, 1, 3], np.uint32))
        with pytest.raises(sge.SgeError, match="mesh id out of range"):
            _upload(gpu, sge.abi.SGE_MAX_SCENE_MESHES, tri)
        with pytest.raises(sge.SgeError, match="never uploaded"):
            gpu.scene_mesh_info(0)
        with pytest.raises(sge.SgeError, match="never uploaded"):
            gpu.scene_instances([0], columns(np.eye(4)[None]))
        _upload(gpu, 0, tri)
        _upload(gpu, sge.abi.SGE_MAX_SCENE_MESHES - 1, rib)
        mats = np.tile(np.eye(4, dtype=np.float32), (2, 1, 1))
        mats[1][:3, 3] = (0, 5, 0)
        mesh_of = [0, sge.abi.SGE_MAX_SCENE_MESHES - 1]
        gpu.scene_instances(mesh_of, columns(mats))
        ref = SceneRef(sge, {0: tri, sge.abi.SGE_MAX_SCENE_MESHES - 1: rib}, mesh_of, mats)
        rng = np.random.default_rng(3)
        O, D = zip(*[_rays_at(rng, np.array(lo, np.float32), np.array(hi, np.float32), 150) for lo, hi in (((-0.4, -0.4, -0.1), (0.4, 0.4, 0.1)), ((0, 5, -1), (16, 5.5, 1)))])
        O, D = np.concatenate(O), np.concatenate(D)
        base = gpu.scene_intersect(O, D, -1)
        assert_records_match(base, ref.intersect(O, D, -1), "contract scene")
        assert base["hit"].sum() > 60
        # a failed sge_scene_instances_set / _update leaves the previous scene traceable
        bad = columns(mats).copy()
        for poison, match in ((np.nan, "non-finite"), (np.inf, "non-finite")):
            b = bad.copy(); b[1, 5] = poison
            with pytest.raises(sge.SgeError, match=match):
                gpu.scene_instances(mesh_of, b)
            with pytest.raises(sge.SgeError, match=match):
                gpu.scene_instances_update(b[1:], first=1)
        flat = bad.copy(); flat[0, 8:11] = 0  # a zero column: determinant 0
        with pytest.raises(sge.SgeError, match="not invertible"):
            gpu.scene_instances(mesh_of, flat)
        with pytest.raises(sge.SgeError, match="not invertible"):
            gpu.scene_instances_update(flat[:1], first=0)
        with pytest.raises(sge.SgeError, match="never uploaded"):
            gpu.scene_instances([0, 7], bad)
        with pytest.raises(sge.SgeError, match="out of range"):
            gpu.scene_instances_update(bad, first=1)
        with pytest.raises(sge.SgeError, match="bad argument"):
            gpu.scene_instances_update(bad[:1], first=-1)
        too_many = sge.abi.SGE_MAX_SCENE_INSTANCES + 1
        ident = np.tile(np.eye(4, dtype=np.float32).reshape(16), (too_many, 1))
        with pytest.raises(sge.SgeError, match="code %d.*SGE_MAX_SCENE_INSTANCES" % sge.abi.SGE_ERR_INVALID):
            gpu.scene_instances(np.zeros(too_many, np.int32), ident)
        assert gpu.scene_info().staticInstances == 2
        assert gpu.scene_intersect(O, D, -1).tobytes() == base.tobytes()
        # uploading again a mesh in use changes later hits accordingly
        big = dict(tri); big["positions"] = (tri["positions"] * 3).astype(np.float32)
        _upload(gpu, 0, big)
        ref.close()
        ref = SceneRef(sge, {0: big, sge.abi.SGE_MAX_SCENE_MESHES - 1: rib}, mesh_of, mats)
        o = np.array([[1.0, -1.0, -3]], np.float32)  # outside the small triangle, inside the large one
        assert base["hit"].sum() > 0 and gpu.scene_intersect(o, [[0, 0, 1]], -1)["hit"].tolist() == [1]
        assert_records_match(gpu.scene_intersect(O, D, -1), ref.intersect(O, D, -1), "after the re-upload")
        assert gpu.scene_occluded(o, [[0, 0, 1]], -1).tolist() == [1]
        # clearing
        gpu.scene_instances([], np.zeros((0, 16), np.float32))
        assert gpu.scene_info().staticInstances == 0 and gpu.scene_intersect(O, D, -1)["hit"].sum() == 0
    finally:
        gpu.close()
        if ref is not None:
            ref.close()


def test_a_context_with_mesh_variants_traces_the_statics_only(sge):
    gpu = sge.CharacterEngine(0)
    try:
        build_scene(sge, gpu, 2, terrain_cells=(24, 16), rings=9, segments=8, seed=5)
        gpu.blas_build(gpu.mesh["indices"])
        gpu.tick(stages=sge.abi.STAGE_ALL | sge.abi.STAGE_BLAS_REFIT)
        assert gpu.scene_info().crowdReady == 1
        # a ray along the normal of triangle 0 of character 0, from 20 units out: it hits the crowd
        p = gpu.skinned()[0][:gpu.vertex_count].astype(np.float64)
        a, b, c = p[gpu.mesh["indices"].reshape(-1, 3)[0]]
        nrm = np.cross(b - a, c - a); nrm /= np.linalg.norm(nrm)
        ctr = (a + b + c) / 3
        o, d = (ctr + nrm * 20).astype(np.float32)[None], (-nrm).astype(np.float32)[None]
        first = gpu.scene_intersect(o, d, -1)
        assert first["hit"].tolist() == [1] and 0 <= first["instance"][0] < 2, "the crowd is traced until a variant is uploaded"
        gpu.upload_mesh_variant(1, gpu.mesh)
        info = gpu.scene_info()
        assert info.crowdReady == 0 and info.characters == 2
        # a static triangle across the ray, half way
        u = np.cross(nrm, (1, 0, 0) if abs(nrm[0]) < 0.9 else (0, 1, 0)); u /= np.linalg.norm(u)
        v = np.cross(nrm, u)
        q = ctr + nrm * 10
        blocker = _dress(np.array([q + u, q - 0.5 * u + 0.8 * v, q - 0.5 * u - 0.8 * v], np.float32), [0, 1, 2], 5)
        _upload(gpu, 0, blocker)
        gpu.scene_instances([0], columns(np.eye(4, dtype=np.float32)[None]))
        o2, d2 = np.repeat(o, 2, 0), np.repeat(d, 2, 0)
        g = gpu.scene_intersect(o2, d2, [-1, 0])
        assert g["hit"].tolist() == [1, 0] and g["instance"].tolist() == [STATIC_BASE, -1]
        assert abs(g["distance"][0] - 10) < 1e-3
        assert gpu.scene_occluded(o2, d2, [-1, 0]).tolist() == [1, 0]
    finally:
        gpu.close()
