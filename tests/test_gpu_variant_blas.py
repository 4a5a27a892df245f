"""Acceleration-structure refit and ray queries for a crowd with mesh variants (include/sge_amd_variant_blas.h;
csrc/sge_blas_variants.hip) on the GPU.

The reference throughout is the uniform path: for every variant v a second context holds v's mesh as its ONLY mesh, with the same
skeleton, characters, palettes and instance matrices, and is ticked with SGE_STAGE_SKIN | SGE_STAGE_BLAS_REFIT in the two-launch
form. tests/test_gpu_mesh_variants.py pins the skinned bytes of the two paths as identical and a refit is min / max of those
bytes, so boxes compare BIT FOR BIT, and so do the hit records of rays that name their character (both closest-hit kernels are the
same expression tree, compiled in translation units with the same contraction setting).

Shapes: 37 characters, 65 bones, both output layouts, four variants, each a complete mesh with its own index buffer:
  variant 0   9,001 vertices (odd), 9,000 triangles   three tiles of 3,008 with a partial last one; > 4,096 triangles: two wide levels
  variant 1   1,001 vertices (odd), 1,200 triangles   one tile; triangles 999.. repeat earlier ones' vertices in another order
  variant 2       3 vertices,           1 triangle    the smallest structure there is
  variant 3     300 vertices,         500 triangles   one tile, even
so that behind any character of variant 0, 1 or 2 the next one starts at an odd vertex offset."""
import ctypes as C
import functools

import numpy as np
import pytest

from blas_ref import expected_bounds
from scenes import _SyntheticRig, build_scene
from skin_ref import make_skin_case, rigid_shear_palette

pytestmark = pytest.mark.gpu

BONES = 65
CHARS = 37
SHAPES = ((9001, 9000), (1001, 1200), (3, 1), (300, 500))  # (vertices, triangles) per variant
NV = len(SHAPES)
SENTINEL = 7.0


@functools.lru_cache(maxsize=None)
def _hip():
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    return hip


@functools.lru_cache(maxsize=None)
def _rig():
    return _SyntheticRig(BONES, 4, seed=500 + BONES, animate_all=True, translate_some=True)


@functools.lru_cache(maxsize=None)
def _mesh(v):
    V, T = SHAPES[v]
    case = make_skin_case(V, BONES, seed=7000 + v)
    k = np.arange(T, dtype=np.int64)
    strip = np.stack([k, k + 1, k + 2], 1) % V
    wrapped = np.stack([k, k + 7, k + 19], 1) % V
    tri = np.where((k < V - 2)[:, None], strip, wrapped)
    assert (tri[:, 0] != tri[:, 1]).all() and (tri[:, 1] != tri[:, 2]).all() and (tri[:, 0] != tri[:, 2]).all()
    case["indices"] = tri.astype(np.uint32).reshape(-1)
    case["uvs"] = np.random.default_rng(70 + v).uniform(0, 1, (V, 2)).astype(np.float32)
    for a in case.values():
        a.setflags(write=False)
    return case


@functools.lru_cache(maxsize=None)
def _palettes(seed=5):
    rng = np.random.default_rng(seed)
    pal = np.stack([rigid_shear_palette(BONES, rng, translation=30.0) for _ in range(CHARS)])
    pal[5] = pal[4]  # characters 4 and 5 stand at the same place (same instance matrix below): see the any-instance test
    pal.setflags(write=False)
    return pal


@functools.lru_cache(maxsize=None)
def _instances():
    """[CHARS][16] column-major: spread along x, one rotated, one scaled non-uniformly; 4 and 5 share a matrix."""
    m = np.tile(np.eye(4, dtype=np.float32), (CHARS, 1, 1))
    m[:, 0, 3] = np.arange(CHARS) * 35.0
    m[:, 2, 3] = (np.arange(CHARS) % 5) * 20.0
    m[5] = m[4]
    m[7][:3, :3] = np.diag([1.5, 0.75, 2.0]).astype(np.float32) @ np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], np.float32)
    m.setflags(write=False)
    return m


def _cols(m):
    return np.ascontiguousarray(m.transpose(0, 2, 1)).reshape(len(m), 16)


def _patterns():
    blocks = np.minimum(np.arange(CHARS) // 10, NV - 1)
    one_empty = np.array([0, 2, 3])[np.arange(CHARS) % 3]
    single = np.where(np.arange(CHARS) % 2 == 0, 1, 3)
    single[20] = 0                                                  # a single character in the largest mesh
    mixed = np.arange(CHARS) % NV
    mixed[4], mixed[5] = 0, 1                                       # different variants at the same place
    return {"all in variant 1": np.full(CHARS, 1), "all in the largest": np.zeros(CHARS, np.int64), "round robin": np.arange(CHARS) % NV,
            "blocks": blocks, "variant 1 empty": one_empty, "one character in the largest": single, "mixed": mixed}


class _Ctx:
    """A context over the synthetic rig with `variants` (indices into SHAPES) as its meshes 0, 1, ... and CHARS characters."""

    def __init__(self, sge, layout, variants, overlap=0, build=True):
        A = sge.abi
        self.sge, self.A, self.layout, self.variants = sge, A, layout, list(variants)
        self.eng = eng = sge.CharacterEngine(0)
        try:
            eng.set_option(A.OPT_PLACEMENT_PROBES, 1)
            eng.set_option(A.OPT_SKIN_LAYOUT, A.LAYOUT_PADDED16 if layout == "padded16" else A.LAYOUT_PACKED)
            eng.set_option(A.OPT_OVERLAP_SKIN, overlap)
            eng.set_option(A.OPT_FUSE_BLAS_REFIT, 0)  # the reference is the two-launch form
            rig = _rig()
            eng.upload_skeleton(rig)
            eng.upload_profiles(rig.profiles)
            eng.upload_skinned_mesh(_mesh(self.variants[0]))
            for k, v in enumerate(self.variants[1:], 1):
                eng.upload_mesh_variant(k, _mesh(v))
            sge.crowd.spawn_crowd(eng, rig, CHARS, None, mode="lbs")
            if build:
                self.build()
        except BaseException:
            eng.close()
            raise

    def build(self):
        eng = self.eng
        self.info = [eng.blas_build(_mesh(self.variants[0])["indices"])]
        eng.blas_set_uvs(_mesh(self.variants[0])["uvs"])
        for k, v in enumerate(self.variants[1:], 1):
            self.info.append(eng.blas_variant_build(k, _mesh(v)["indices"]))
            eng.blas_variant_set_uvs(k, _mesh(v)["uvs"])
        eng.blas_instances(_cols(_instances()))

    def write_palettes(self, pal):
        self.eng.synchronize()
        p = C.c_void_p()
        self.eng._call("crowd_buffers", C.byref(p), None, None, None)
        pal = np.ascontiguousarray(pal, np.float32)
        assert _hip().hipMemcpy(p, pal.ctypes.data, pal.nbytes, 1) == 0

    def tick(self, refit=True):
        self.eng.tick(dt=0.0, stages=self.A.STAGE_SKIN | (self.A.STAGE_BLAS_REFIT if refit else 0))


def _tiles(V, info):
    """Tiles of the refit schedule by the rule of HostBlas::build: the largest tile capacity of 4,096 / 3,072 / 2,048 vertices that
    lets three workgroups share 160 KB, tiles of equal size rounded up to 64 vertices -> (tile count, vertices in the last tile)."""
    cap = 4096
    for c in (4096, 3072, 2048):
        lds = (info.entryCount + 1) * 24 + c * 12 + (V // c + 3) * 4 + (info.levels + 2 * info.wideCount + 2) * 4 + 16
        if 3 * (lds + 256) <= 160 * 1024:
            cap = c
            break
    n = -(-V // cap)
    tv = (-(-V // n) + 63) // 64 * 64
    n = -(-V // tv)
    return n, V - (n - 1) * tv, tv


@pytest.fixture(scope="module", params=["packed", "padded16"])
def world(sge, request):
    """(variant context, uniform contexts per variant, their boxes under the shared palettes)."""
    layout = request.param
    uniform = [_Ctx(sge, layout, [v]) for v in range(NV)]
    ctx = None
    try:
        boxes = []
        for u in uniform:
            u.write_palettes(_palettes())
            u.tick()
            b = u.eng.blas_bounds()
            b.setflags(write=False)
            boxes.append(b)
        ctx = _Ctx(sge, layout, range(NV))
        ctx.write_palettes(_palettes())
        yield ctx, uniform, boxes
    finally:
        for c in uniform + ([ctx] if ctx else []):
            c.eng.close()


def _check_boxes(ctx, boxes, assign, what, kept=None):
    got, rec = ctx.eng.blas_variant_bounds()
    kept = np.ones(CHARS, bool) if kept is None else kept
    assert np.array_equal(rec, np.where(kept, assign, ctx.A.NO_VARIANT)), (what, rec.tolist())
    for c in np.flatnonzero(kept):
        v = int(assign[c])
        rows = ctx.info[v].entryCount + 1
        same = got[c, :rows].view(np.uint32) == boxes[v][c].view(np.uint32)
        assert same.all(), (what, "character", c, "variant", v, "first differing rows", np.argwhere(~same)[:4].tolist())
    return got


def test_the_shapes_are_the_ones_the_kernels_branch_on(world):
    ctx, uniform, _ = world
    lay = ctx.eng.blas_variant_layout()
    assert lay.ready == 1 and lay.variants == NV and lay.rowStride == max(i.entryCount for i in ctx.info) + 1
    assert list(lay.entryCount)[:NV] == [i.entryCount for i in ctx.info] and list(lay.entryCount)[NV:] == [0] * (8 - NV)
    for v, (V, T) in enumerate(SHAPES):
        info = ctx.eng.blas_variant_info(v)
        assert (info.triangleCount, info.entryCount) == (T, uniform[v].info[0].entryCount)
    tiles = [_tiles(V, ctx.info[v]) for v, (V, _) in enumerate(SHAPES)]
    assert tiles[0][0] == 3 and 0 < tiles[0][1] < tiles[0][2], "several tiles, a partial last one"
    assert tiles[1][0] == tiles[2][0] == tiles[3][0] == 1, "single-tile meshes"
    assert ctx.info[0].triangleCount > 4096 and ctx.info[0].levels >= 2, "two wide levels"
    assert ctx.info[2].triangleCount == 1 and SHAPES[2][0] == 3
    assert SHAPES[0][0] % 2 == 1 and SHAPES[1][0] % 2 == 1, "odd vertex counts: later characters start at odd offsets"


def test_boxes_of_a_tick_with_skin_and_refit(world):
    ctx, uniform, boxes = world
    eng = ctx.eng
    for name, assign in _patterns().items():
        eng.set_mesh_variants(assign)
        ctx.tick()
        got = _check_boxes(ctx, boxes, assign, name)
        if name == "round robin":
            off = eng.vertex_offsets()
            assert (off[1:CHARS] % 2 == 1).any(), "some character starts at an odd vertex"
            pos = eng.skinned(0, int(off[-1]))[0]
            for c in range(CHARS):
                v = int(assign[c])
                topo = ctx.sge.CharacterEngine.blas_topology(_mesh(v)["positions"], _mesh(v)["indices"])
                want = expected_bounds(topo, _mesh(v)["indices"], pos[off[c]:off[c + 1]])
                assert np.array_equal(got[c, :want.shape[0]], want), (c, v)


def test_refit_alone_and_bytes_changed_behind_the_tick(world):
    ctx, uniform, boxes = world
    eng, A = ctx.eng, ctx.A
    assign = _patterns()["mixed"]
    eng.set_mesh_variants(assign)
    ctx.tick(refit=False)
    eng.set_mesh_variants(_patterns()["blocks"])        # behind the tick: the next launch's, not this one's
    eng.blas_refit()
    _check_boxes(ctx, boxes, assign, "sge_blas_refit(0, all) alone")
    eng.tick(dt=0.0, stages=A.STAGE_BLAS_REFIT)
    _check_boxes(ctx, boxes, assign, "SGE_STAGE_BLAS_REFIT alone")
    eng.set_mesh_variants(assign)
    ctx.tick()
    eng.lod_select((0.0, 0.0, 0.0), [1.0])               # the live bytes change; boxes and records describe the launch that ran
    _check_boxes(ctx, boxes, assign, "after a later sge_lod_select")
    # named rays still answer from the launch that ran
    O, D, I = _named_rays(ctx, uniform, assign, per_char=8)
    _same_hits(ctx.eng.blas_intersect(O, D, I), _uniform_named(uniform, assign, O, D, I), "after a later sge_lod_select")


def test_capacity_cut_inside_a_slice(world):
    ctx, uniform, boxes = world
    eng, A = ctx.eng, ctx.A
    assign = _patterns()["mixed"]
    counts = np.array([SHAPES[v][0] for v in assign], np.int64)
    off = np.concatenate([[0], np.cumsum(counts)])
    k = int(np.flatnonzero(assign[20:] == 0)[0]) + 20
    capacity = int(off[k]) + 5
    kept = off[1:] <= capacity
    assert 0 < kept.sum() < CHARS and not kept[k] and kept[k - 1] and kept[k + 1:].sum() == 0
    lay = eng.blas_variant_layout()
    bp = C.c_void_p()
    eng._call("blas_variant_buffers", C.byref(bp), None, None)
    try:
        eng.reserve_vertices(capacity)
        eng.synchronize()
        fill = np.full((CHARS, lay.rowStride, 6), SENTINEL, np.float32)
        assert _hip().hipMemcpy(bp, fill.ctypes.data, fill.nbytes, 1) == 0
        eng.set_mesh_variants(assign)
        ctx.tick()
        assert eng.skin_plan().dropped == CHARS - kept.sum()
        got = _check_boxes(ctx, boxes, assign, "capacity cut", kept)
        assert (got[~kept] == SENTINEL).all(), "the rows of dropped characters are untouched"
        for c in np.flatnonzero(kept):
            assert (got[c, ctx.info[int(assign[c])].entryCount + 1:] == SENTINEL).all(), "rows beyond a variant's own are never written"
        O, D, I = _named_rays(ctx, uniform, assign, per_char=6)
        g = eng.blas_intersect(O, D, I)
        u = _uniform_named(uniform, assign, O, D, I)
        dropped_ray = ~kept[I]
        assert dropped_ray.any() and (g["hit"][dropped_ray] == 0).all() and (g["instance"][dropped_ray] == -1).all()
        _same_hits(g[~dropped_ray], u[~dropped_ray], "kept characters beside dropped ones")
        ga = eng.blas_intersect(O, D, np.full(len(O), -1, np.int32))
        want = _compose(uniform, assign, O, D, kept)
        assert not np.isin(ga["instance"], np.flatnonzero(~kept)).any(), "any-instance rays never report a dropped character"
        for f in ("hit", "instance", "primitive"):
            assert np.array_equal(ga[f], want[f]), f
        assert ga["hit"].any()
    finally:
        eng.reserve_vertices(0)


def test_a_skin_stage_without_a_refit_leaves_no_record_behind(world):
    """skin + refit, then skin ONLY under another assignment and a reservation that drops characters: the offsets in place are the
    new plan's, the boxes the old one's, so no character has a structure until the next refit. Named rays and rays without an
    instance must all miss (a kernel that paired an old record with a new offset would walk another character's vertices, or
    read past the reserved capacity); the boxes are untouched; a refit alone then describes the NEW launch."""
    ctx, uniform, boxes = world
    eng, A = ctx.eng, ctx.A
    first, second = _patterns()["mixed"], _patterns()["blocks"]
    assert (first != second).any()
    eng.set_mesh_variants(first)
    ctx.tick()
    before, rec = eng.blas_variant_bounds()
    assert np.array_equal(rec, first)
    O, D, I = _named_rays(ctx, uniform, first, per_char=4)
    assert eng.blas_intersect(O, D, I)["hit"].any()
    counts = np.array([SHAPES[v][0] for v in second], np.int64)
    off = np.concatenate([[0], np.cumsum(counts)])
    capacity = int(off[30]) + 1                                   # inside character 30's slice: 30.. are dropped
    kept = off[1:] <= capacity
    assert kept.sum() == 30
    try:
        eng.reserve_vertices(capacity)
        eng.set_mesh_variants(second)
        ctx.tick(refit=False)
        after, rec = eng.blas_variant_bounds()
        assert (rec == A.NO_VARIANT).all(), rec.tolist()
        assert np.array_equal(after.view(np.uint32), before.view(np.uint32)), "a skin stage alone writes no box"
        g = eng.blas_intersect(O, D, I)
        assert (g["hit"] == 0).all() and (g["instance"] == -1).all() and (g["primitive"] == -1).all()
        g = eng.blas_intersect(O, D, np.full(len(O), -1, np.int32))
        assert (g["hit"] == 0).all() and (g["instance"] == -1).all()
        eng.blas_refit()
        _check_boxes(ctx, boxes, second, "refit alone behind a skin-only tick", kept)
        Ok, Dk, Ik = _named_rays(ctx, uniform, second, per_char=4)
        g, u = eng.blas_intersect(Ok, Dk, Ik), _uniform_named(uniform, second, Ok, Dk, Ik)
        assert (g["hit"][~kept[Ik]] == 0).all() and g["hit"][kept[Ik]].any()
        _same_hits(g[kept[Ik]], u[kept[Ik]], "after the refit")
    finally:
        eng.reserve_vertices(0)


def _world_positions(ctx, uniform, assign, c):
    v = int(assign[c])
    V = SHAPES[v][0]
    p = uniform[v].eng.skinned(c * V, V)[0]
    m = _instances()[c]
    return p @ m[:3, :3].T + m[:3, 3]


def _rays_at(rng, lo, hi, k):
    centre, half = (lo + hi) / 2, (hi - lo) / 2
    d = rng.normal(size=(k, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    origins = centre + d * (np.linalg.norm(half) * rng.uniform(1.2, 3.0, (k, 1)))
    targets = centre + rng.uniform(-1, 1, (k, 3)) * half
    dirs = targets - origins
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    return origins.astype(np.float32), dirs.astype(np.float32)


def _named_rays(ctx, uniform, assign, per_char, seed=11):
    """Rays that name their character: from a shell around it towards points inside its box, exactly through vertices and edge
    midpoints, and from inside."""
    rng = np.random.default_rng(seed)
    O, D, I = [], [], []
    for c in range(CHARS):
        world = _world_positions(ctx, uniform, assign, c)
        lo, hi = world.min(0) - 1e-3, world.max(0) + 1e-3
        o, d = _rays_at(rng, lo, hi, per_char)
        tri = _mesh(int(assign[c]))["indices"].reshape(-1, 3)
        tri = tri[rng.integers(0, len(tri), 4)]
        tgt = np.concatenate([world[tri[:2, 0]], (world[tri[2:, 0]] + world[tri[2:, 1]]) / 2]).astype(np.float32)
        centre = world.mean(0) + 0.37
        o2 = (centre + (tgt - centre) * 4).astype(np.float32)
        d2 = tgt - o2
        o3 = ((lo + hi) / 2 + rng.uniform(-0.2, 0.2, (2, 3)) * (hi - lo)).astype(np.float32)  # start inside the box
        d3 = rng.normal(size=(2, 3)).astype(np.float32)
        for oo, dd in ((o, d), (o2, d2), (o3, d3)):
            O.append(oo.astype(np.float32)); D.append((dd / np.linalg.norm(dd, axis=1, keepdims=True)).astype(np.float32))
            I.append(np.full(len(oo), c, np.int32))
    return np.concatenate(O), np.concatenate(D), np.concatenate(I)


def _uniform_named(uniform, assign, O, D, I):
    """The uniform contexts' answers: ray i from the context of the variant of character I[i]."""
    out = np.zeros(len(O), uniform[0].A.blas_hit_dtype)
    for v in range(NV):
        sel = np.flatnonzero(assign[I] == v)
        if len(sel):
            out[sel] = uniform[v].eng.blas_intersect(O[sel], D[sel], I[sel])
    return out


def _same_hits(got, want, what):
    assert got.shape == want.shape
    for f in got.dtype.names:
        g, w = np.ascontiguousarray(got[f]), np.ascontiguousarray(want[f])
        same = g.view(np.uint32) == w.view(np.uint32)
        assert same.all(), (what, f, "first differing rays", np.argwhere(~same)[:4].tolist())


def _compose(uniform, assign, O, D, kept=None):
    """Closest hit over all characters from the uniform contexts' named answers: smallest distance bits, then smaller instance."""
    n = len(O)
    best = np.full(n, np.iinfo(np.uint64).max, np.uint64)
    out = {"hit": np.zeros(n, np.int32), "instance": np.full(n, -1, np.int32), "primitive": np.full(n, -1, np.int32)}
    for v in range(NV):
        chars = [c for c in range(CHARS) if assign[c] == v and (kept is None or kept[c])]
        if not chars:
            continue
        I = np.repeat(np.array(chars, np.int32), n)
        h = uniform[v].eng.blas_intersect(np.tile(O, (len(chars), 1)), np.tile(D, (len(chars), 1)), I).reshape(len(chars), n)
        for k, c in enumerate(chars):
            key = (h["distance"][k].view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(c)
            take = (h["hit"][k] == 1) & (key < best)
            best[take] = key[take]
            out["hit"][take], out["instance"][take], out["primitive"][take] = 1, c, h["primitive"][k][take]
    return out


def test_named_rays_are_bit_identical_to_the_uniform_contexts(world):
    ctx, uniform, boxes = world
    assign = _patterns()["mixed"]
    ctx.eng.set_mesh_variants(assign)
    ctx.tick()
    O, D, I = _named_rays(ctx, uniform, assign, per_char=24)
    per_variant = [int((assign[I] == v).sum()) for v in range(NV)]
    assert min(per_variant) >= 200, per_variant
    got = ctx.eng.blas_intersect(O, D, I)
    want = _uniform_named(uniform, assign, O, D, I)
    assert got["hit"].sum() > 0.2 * len(O) and (got["hit"] == 0).any(), "a condition, not a measurement: the rays are aimed"
    scaled = I == 7
    assert got["hit"][scaled].any(), "the scaled instance is hit"
    _same_hits(got, want, "named rays")
    hit = got["hit"] == 1
    assert (got["primitive"][hit] < np.array([SHAPES[v][1] for v in assign[I[hit]]])).all()
    assert (got["uv"][hit] != 0).any()


def test_rays_without_an_instance_compose_the_uniform_answers(world):
    import torch
    ctx, uniform, boxes = world
    eng, A = ctx.eng, ctx.A
    assign = _patterns()["mixed"]
    assert assign[4] != assign[5] and np.array_equal(_instances()[4], _instances()[5]) and np.array_equal(_palettes()[4], _palettes()[5])
    eng.set_mesh_variants(assign)
    ctx.tick()
    O, D, I = _named_rays(ctx, uniform, assign, per_char=2, seed=13)
    at45 = (I == 4) | (I == 5)
    O, D = np.concatenate([O[at45], O[~at45][::3]]), np.concatenate([D[at45], D[~at45][::3]])
    want = _compose(uniform, assign, O, D)
    none = np.full(len(O), -1, np.int32)
    got = eng.blas_intersect(O, D, none)
    for f in ("hit", "instance", "primitive"):
        assert np.array_equal(got[f], want[f]), (f, np.argwhere(got[f] != want[f])[:4].tolist())
    assert got["hit"].sum() > 0.2 * len(O) and len(set(assign[got["instance"][got["hit"] == 1]].tolist())) >= 2
    # the device entry point gives the same records
    rays = np.zeros(len(O), A.blas_ray_dtype)
    rays["origin"], rays["direction"], rays["minDistance"], rays["maxDistance"], rays["instance"] = O, D, 0.001, 1e6, none
    d_rays = torch.from_numpy(rays.view(np.uint8)).to("cuda:0")
    d_hits = torch.zeros(len(O) * A.blas_hit_dtype.itemsize, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    eng.blas_intersect_device(d_rays.data_ptr(), len(O), d_hits.data_ptr(), any_instance=True)
    eng.synchronize()
    _same_hits(d_hits.cpu().numpy().view(A.blas_hit_dtype), got, "device entry point")
    # any_instance = 0 with a ray that breaks the promise: a miss
    d_hits.zero_()
    torch.cuda.synchronize()
    eng.blas_intersect_device(d_rays.data_ptr(), len(O), d_hits.data_ptr(), any_instance=False)
    eng.synchronize()
    assert (d_hits.cpu().numpy().view(A.blas_hit_dtype)["hit"] == 0).all()


def test_contract(sge):
    ctx = _Ctx(sge, "packed", range(NV), build=False)
    try:
        eng, lib, A = ctx.eng, ctx.eng.t.lib, ctx.A
        idx = [_mesh(v)["indices"] for v in range(NV)]
        d = A.TickDesc()
        d.dt = 0.0

        def refused():
            d.stages, d.first, d.count = A.STAGE_SKIN | A.STAGE_BLAS_REFIT, 0, 0
            assert lib.sge_tick(eng.h, C.byref(d)) == A.SGE_ERR_STATE and b"variant" in lib.sge_last_error()
            assert lib.sge_blas_refit(eng.h, 0, CHARS) == A.SGE_ERR_STATE and b"variant" in lib.sge_last_error()
            rays, hits = np.zeros(1, A.blas_ray_dtype), np.zeros(1, A.blas_hit_dtype)
            assert lib.sge_blas_intersect_batch(eng.h, A.ptr(rays), 1, A.ptr(hits)) == A.SGE_ERR_STATE and b"variant" in lib.sge_last_error()
            assert lib.sge_blas_intersect_device(eng.h, C.c_void_p(16), 1, C.c_void_p(16), 1) == A.SGE_ERR_STATE and b"variant" in lib.sge_last_error()
            assert lib.sge_blas_variant_bounds_download(eng.h, 0, CHARS, None, None) == A.SGE_ERR_STATE
            assert lib.sge_blas_variant_buffers(eng.h, None, None, None) == A.SGE_ERR_STATE
            assert eng.blas_variant_layout().ready == 0 and eng.blas_variant_layout().rowStride == 0

        refused()
        assert lib.sge_blas_variant_build(eng.h, 1, A.ptr(idx[1]), idx[1].size) == A.SGE_ERR_STATE, "before sge_blas_build"
        eng.blas_build(idx[0])
        refused()
        assert lib.sge_blas_variant_build(eng.h, 0, A.ptr(idx[0]), idx[0].size) == A.SGE_ERR_INVALID, "variant 0: sge_blas_build"
        assert lib.sge_blas_variant_build(eng.h, NV, A.ptr(idx[1]), idx[1].size) == A.SGE_ERR_INVALID, "never uploaded"
        assert lib.sge_blas_variant_build(eng.h, 1, A.ptr(idx[1]), 0) == A.SGE_ERR_INVALID, "no triangles"
        bad = idx[1].copy()
        bad[5] = SHAPES[1][0]
        assert lib.sge_blas_build(eng.h, A.ptr(np.array([0, 1, SHAPES[0][0]], np.uint32)), 3) == lib.sge_blas_variant_build(eng.h, 1, A.ptr(bad), bad.size) == A.SGE_ERR_INVALID
        eng.blas_build(idx[0])
        for v in range(1, NV):
            refused()
            eng.blas_variant_build(v, idx[v])
        assert eng.blas_variant_layout().ready == 1
        assert lib.sge_blas_refit(eng.h, 0, CHARS) == A.SGE_ERR_STATE and b"skin stage" in lib.sge_last_error(), "before any skin stage"
        ctx.write_palettes(_palettes())
        eng.set_mesh_variants(_patterns()["round robin"])
        ctx.tick()
        eng.blas_refit()
        eng.tick(dt=0.0, stages=A.STAGE_BLAS_REFIT)
        bounds, rec = eng.blas_variant_bounds()
        assert np.array_equal(rec, _patterns()["round robin"]) and np.isfinite(bounds[:, 0]).all()
        O, D, I = np.zeros((1, 3), np.float32), np.array([[1, 0, 0]], np.float32), np.array([3], np.int32)
        eng.blas_intersect(O, D, I)
        eng.blas_instances(_cols(_instances()))
        assert lib.sge_blas_refit(eng.h, 3, 10) == A.SGE_ERR_STATE and b"whole crowd" in lib.sge_last_error()
        d.stages, d.first, d.count = A.STAGE_BLAS_REFIT, 3, 10
        assert lib.sge_tick(eng.h, C.byref(d)) == A.SGE_ERR_STATE and b"whole crowd" in lib.sge_last_error()
        assert lib.sge_blas_refit_buffers(eng.h, C.c_void_p(16), A.LAYOUT_PACKED, 0, 1, C.c_void_p(16)) == A.SGE_ERR_STATE and b"variant" in lib.sge_last_error()
        out = np.zeros((CHARS, 4096, 6), np.float32)
        assert lib.sge_blas_bounds_download(eng.h, 0, CHARS, A.ptr(out)) == A.SGE_ERR_STATE and b"sge_blas_variant_bounds_download" in lib.sge_last_error()
        ptrs = (C.c_void_p * 8)()
        bp, cp = C.c_void_p(), C.c_void_p()
        eng._call("blas_variant_buffers", C.byref(bp), C.byref(cp), ptrs)
        assert bp.value and cp.value and all(ptrs[v] for v in range(NV)) and not any(ptrs[v] for v in range(NV, 8))
        # a variant upload (replacing one) makes the context not ready again; so does sge_blas_build alone
        eng.upload_mesh_variant(2, _mesh(2))
        refused()
        eng.blas_variant_build(2, idx[2])
        assert eng.blas_variant_layout().ready == 1
        eng.blas_build(idx[0])
        refused()
        # after sge_characters_resize every record is 0xFF
        for v in range(1, NV):
            eng.blas_variant_build(v, idx[v])
        eng.resize(CHARS)
        assert (eng.blas_variant_bounds()[1] == A.NO_VARIANT).all()
    finally:
        ctx.eng.close()


TICKS = 6


def _scene_ctx(sge, overlap, variants):
    A = sge.abi
    eng = sge.CharacterEngine(0)
    try:
        eng.set_option(A.OPT_PLACEMENT_PROBES, 1)
        eng.set_option(A.OPT_OVERLAP_SKIN, overlap)
        eng.set_option(A.OPT_FUSE_BLAS_REFIT, 0)
        build_scene(sge, eng, CHARS, terrain_cells=(32, 24), seed=3, pose_debug=False)
        eng.upload_skinned_mesh(_mesh(variants[0]))
        for k, v in enumerate(variants[1:], 1):
            eng.upload_mesh_variant(k, _mesh(v))
        eng.blas_build(_mesh(variants[0])["indices"])
        for k, v in enumerate(variants[1:], 1):
            eng.blas_variant_build(k, _mesh(v)["indices"])
    except BaseException:
        eng.close()
        raise
    return eng


def test_six_ticks_with_changing_assignments_under_every_overlap_mode(sge):
    """Overlap 0, 1 and 2, all on a caller's stream, no host synchronisation in the loop: a consumer stream ordered by sge_skin_wait
    copies boxes and records device to device. The reference boxes come from uniform contexts fed the palettes of a serial run."""
    import torch
    A = sge.abi
    rng = np.random.default_rng(3)
    assigns = [rng.integers(0, NV, CHARS) for _ in range(TICKS)]
    st = A.STAGE_ALL | A.STAGE_BLAS_REFIT
    eng = _scene_ctx(sge, 0, list(range(NV)))
    pals = []
    try:
        for a in assigns:
            eng.set_mesh_variants(a)
            eng.tick(stages=st)
            pals.append(eng.palettes()[0])
    finally:
        eng.close()
    assert np.abs(pals[0] - pals[-1]).max() > 1e-3
    want = [[None] * NV for _ in range(TICKS)]
    rows = [0] * NV
    for v in range(NV):
        u = _Ctx(sge, "packed", [v])
        try:
            rows[v] = u.info[0].entryCount + 1
            for t in range(TICKS):
                u.write_palettes(pals[t])
                u.tick()
                want[t][v] = u.eng.blas_bounds()
        finally:
            u.eng.close()
    hip, dev = _hip(), torch.device("cuda", 0)
    for overlap in (0, 1, 2):
        eng = _scene_ctx(sge, overlap, list(range(NV)))
        lib, h = eng.t.lib, eng.h
        try:
            consumer, caller = torch.cuda.Stream(device=0), torch.cuda.Stream(device=0)
            assert lib.sge_context_set_stream(h, C.c_void_p(caller.cuda_stream)) == 0
            bp, cp = C.c_void_p(), C.c_void_p()
            eng._call("blas_variant_buffers", C.byref(bp), C.byref(cp), None)
            stride = eng.blas_variant_layout().rowStride
            copies = []
            for a in assigns:
                eng.set_mesh_variants(a)
                eng.tick(stages=st)
                assert lib.sge_skin_wait(h, C.c_void_p(consumer.cuda_stream)) == 0
                bufs = [torch.empty((CHARS, stride, 6), dtype=torch.float32, device=dev), torch.empty(CHARS, dtype=torch.uint8, device=dev)]
                for b, p in zip(bufs, (bp, cp)):
                    assert hip.hipMemcpyAsync(C.c_void_p(b.data_ptr()), p, b.numel() * b.element_size(), 3, C.c_void_p(consumer.cuda_stream)) == 0
                assert lib.sge_skin_consumed(h, C.c_void_p(consumer.cuda_stream)) == 0
                copies.append(bufs)
            eng.synchronize()
            consumer.synchronize()
            for t, (b, r) in enumerate(copies):
                b, r = b.cpu().numpy(), r.cpu().numpy()
                assert np.array_equal(r, assigns[t]), (overlap, t)
                for c in range(CHARS):
                    v = int(assigns[t][c])
                    assert np.array_equal(b[c, :rows[v]].view(np.uint32), want[t][v][c].view(np.uint32)), (overlap, t, c, v)
            assert lib.sge_context_set_stream(h, None) == 0
        finally:
            eng.close()
