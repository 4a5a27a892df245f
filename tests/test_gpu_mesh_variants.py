"""Per-character mesh variants and distance LOD (include/sge_amd_variants.h; csrc/sge_skin_variants.hip) on the GPU.

Three variants of V = 1000, 257 and 1 vertices (not a multiple of the 256-thread block; one block plus one vertex; a single vertex),
37 characters (no multiple of any CPW, below the 64 characters of the uniform multi-character form), rigs of 65 and 256 bones, both
output layouts. The variant kernel takes at most four characters per unit, and four palettes of 256 bones fit the 64 KiB rule
(4 x 256 x 48 + 16 B), so both rigs run CPW = 4; the 256-bone rig brings bone indices up to 255 and the largest palettes.

The oracle of every byte is the project's own uniform path: a second context that holds ONLY one variant's mesh, is fed the same
palettes and skins through the code path every earlier test pins. Bit identity is derived, not measured: skinVertex
(csrc/sge_skin_vertex.hpp) is the expression tree of skinRange / skinRangeMulti term for term, both translation units are
compiled with the same contraction setting, and a character's bytes depend on its palette and its source vertex alone, not on
the group it was skinned in. The float64 bars of tests/skin_ref.py are applied unchanged on top.

Palettes are skin_ref.rigid_shear_palette matrices written straight into the context's palette buffer (sge_crowd_buffers), and the
tick runs SGE_STAGE_SKIN alone: the pose-free route. The schedule test runs the full stage set and takes the pose stage's palettes."""
import ctypes as C
import functools

import numpy as np
import pytest

from scenes import _SyntheticRig, build_scene
from skin_ref import check_streams, make_skin_case, rigid_shear_palette, skin_reference

pytestmark = pytest.mark.gpu

VS = (1000, 257, 1)
CHARS = 37
LAYOUTS = ["packed", "padded16"]
SENTINEL = 7.0


@functools.lru_cache(maxsize=None)
def _hip():
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    return hip


@functools.lru_cache(maxsize=None)
def _rig(bones):
    return _SyntheticRig(bones, 4, seed=500 + bones, animate_all=True, translate_some=True)


@functools.lru_cache(maxsize=None)
def _case(V, B):
    case = make_skin_case(V, B, seed=1000 * B + V)
    for a in case.values():
        a.setflags(write=False)
    return case


@functools.lru_cache(maxsize=None)
def _palettes(bones, seed=5):
    """[CHARS][bones][16]: every character a palette of its own. Shared and never written to."""
    rng = np.random.default_rng(seed + bones)
    pal = np.stack([rigid_shear_palette(bones, rng, translation=30.0) for _ in range(CHARS)])
    pal.setflags(write=False)
    return pal


def _patterns():
    rng = np.random.default_rng(99)
    one_empty = np.where(np.arange(CHARS) % 2 == 0, 0, 2)
    exactly_one = np.zeros(CHARS, np.int64)
    exactly_one[1::2] = 2
    exactly_one[20] = 1
    return {"all variant 0": np.zeros(CHARS, np.int64), "all in the last": np.full(CHARS, 2), "round robin": np.arange(CHARS) % 3,
            "variant 1 empty": one_empty, "exactly one in variant 1": exactly_one, "seeded random": rng.integers(0, 3, CHARS)}


class _Ctx:
    """A context with `meshes` (variant 0, 1, ...) over the synthetic rig and CHARS characters; raw access to its device buffers."""

    def __init__(self, sge, bones, layout, meshes, overlap=0, populate=True):
        A = sge.abi
        self.sge, self.A, self.bones, self.layout = sge, A, bones, layout
        self.stride = 4 if layout == "padded16" else 3
        self.eng = sge.CharacterEngine(0)
        try:
            self.eng.set_option(A.OPT_PLACEMENT_PROBES, 1)
            self.eng.set_option(A.OPT_SKIN_LAYOUT, A.LAYOUT_PADDED16 if layout == "padded16" else A.LAYOUT_PACKED)
            self.eng.set_option(A.OPT_OVERLAP_SKIN, overlap)
            if populate:
                rig = _rig(bones)
                self.eng.upload_skeleton(rig)
                self.eng.upload_profiles(rig.profiles)
                self.upload_meshes(meshes)
                sge.crowd.spawn_crowd(self.eng, rig, CHARS, None, mode="lbs")
        except BaseException:
            self.eng.close()
            raise

    def upload_meshes(self, meshes):
        self.eng.upload_skinned_mesh(meshes[0])
        for v, m in enumerate(meshes[1:], 1):
            self.eng.upload_mesh_variant(v, m)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.eng.close()

    def pointers(self):
        ptrs = [C.c_void_p() for _ in range(4)]
        self.eng._call("crowd_buffers", *[C.byref(p) for p in ptrs])
        return ptrs  # palettes, positions, normals, tangents

    def write_palettes(self, pal):
        self.eng.synchronize()
        pal = np.ascontiguousarray(pal, np.float32)
        assert _hip().hipMemcpy(self.pointers()[0], pal.ctypes.data, pal.nbytes, 1) == 0  # hipMemcpyHostToDevice

    def fill(self, vertices, value=SENTINEL):
        """`value` in every float of the first `vertices` vertices of the three streams."""
        self.eng.synchronize()
        for p, width in zip(self.pointers()[1:], (self.stride, self.stride, 4)):
            a = np.full((vertices, width), value, np.float32)
            assert _hip().hipMemcpy(p, a.ctypes.data, a.nbytes, 1) == 0

    def streams(self, vertices):
        self.eng.synchronize()
        out = [np.empty((vertices, self.stride), np.float32), np.empty((vertices, self.stride), np.float32), np.empty((vertices, 4), np.float32)]
        for a, p in zip(out, self.pointers()[1:]):
            assert p.value and _hip().hipMemcpy(a.ctypes.data, p, a.nbytes, 2) == 0  # hipMemcpyDeviceToHost
        return out

    def skin(self):
        self.eng.tick(dt=0.0, stages=self.A.STAGE_SKIN)

    def form(self):
        q, cpw = C.c_int32(-1), C.c_int32(-1)
        assert self.eng.t.lib.sge_debug_skin_form(self.eng.h, C.byref(q), C.byref(cpw)) == 0
        return q.value, cpw.value


class _Oracle:
    """One uniform context per variant mesh: run(palettes) -> per variant the three streams as [CHARS][V][width], through the path
    a context without variants has always taken."""

    def __init__(self, sge, bones, layout):
        self.ctx = [_Ctx(sge, bones, layout, [_case(V, bones)]) for V in VS]

    def close(self):
        for c in self.ctx:
            c.eng.close()

    def run(self, pal):
        out = []
        for c, V in zip(self.ctx, VS):
            c.write_palettes(pal)
            c.skin()
            assert c.form() == (0, 1)
            out.append([a.reshape(CHARS, V, -1) for a in c.streams(CHARS * V)])
        return out


def _expect_streams(uniform, assign):
    """The ragged streams the assignment asks for, cut out of the uniform contexts' -> ([total][width] x 3, offsets)."""
    counts = np.array([VS[v] for v in assign], np.int64)
    off = np.concatenate([[0], np.cumsum(counts)])
    parts = [[uniform[v][s][c] for c, v in enumerate(assign)] for s in range(3)]
    return [np.concatenate(p) for p in parts], off


def _assert_bits(got, want, what):
    for g, w, name in zip(got, want, ("positions", "normals", "tangents")):
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        same = g.view(np.uint32) == w.view(np.uint32)
        assert same.all(), (what, name, "first differing vertices", np.argwhere(~same)[:4].tolist())


def _check_float64(bones, pal, assign, got, off, name):
    """The project's bars, unchanged: per variant, its characters' slices against the float64 reference of that variant's mesh."""
    for v, V in enumerate(VS):
        chars = [c for c in range(CHARS) if assign[c] == v]
        if not chars:
            continue
        ref = skin_reference(_case(V, bones), pal[chars])
        rows = np.concatenate([np.arange(off[c], off[c + 1]) for c in chars])
        rp, rd = check_streams(*[g[rows] for g in got], ref, "%s variant %d" % (name, v))
        print("mesh-variants %s variant %d position %.3f direction %.3f" % (name, v, rp, rd))


@pytest.fixture(scope="module", params=[(65, "packed"), (65, "padded16"), (256, "packed"), (256, "padded16")], ids=lambda p: "%d-%s" % p)
def world(sge, request):
    """(variant context, oracle streams of the shared palettes) per rig and layout; the oracle is computed once."""
    bones, layout = request.param
    oracle = _Oracle(sge, bones, layout)
    try:
        uniform = oracle.run(_palettes(bones))
    finally:
        oracle.close()
    ctx = _Ctx(sge, bones, layout, [_case(V, bones) for V in VS])
    ctx.write_palettes(_palettes(bones))
    yield ctx, uniform
    ctx.eng.close()


def test_every_pattern_is_bit_identical_to_the_uniform_forms(world):
    ctx, uniform = world
    pal = _palettes(ctx.bones)
    for name, assign in _patterns().items():
        ctx.eng.set_mesh_variants(assign)
        ctx.skin()
        want, off = _expect_streams(uniform, assign)
        got = ctx.streams(int(off[-1]))
        _assert_bits(got, want, name)
        assert np.array_equal(ctx.eng.vertex_offsets(), off), name
        _check_float64(ctx.bones, pal, assign, got, off, "%d bones %s %s" % (ctx.bones, ctx.layout, name))
        assert ctx.form()[1] == 4, "four characters per unit at 65 and at 256 bones (4 x 256 x 48 + 16 <= 64 KiB)"
    p, n, t = ctx.eng.skinned_character(5)
    c5 = slice(int(off[5]), int(off[6]))
    assert np.array_equal(p, got[0][c5][:, :3]) and np.array_equal(n, got[1][c5][:, :3]) and np.array_equal(t, got[2][c5])


def test_layout_offsets_plan_and_the_room_behind_the_last_character(world):
    ctx, uniform = world
    assign = np.arange(CHARS) % 3
    capacity = CHARS * max(VS)
    ctx.eng.reserve_vertices(0)
    ctx.fill(capacity)
    ctx.eng.set_mesh_variants(assign)
    ctx.skin()
    want, off = _expect_streams(uniform, assign)
    assert np.array_equal(ctx.eng.vertex_offsets(), np.concatenate([[0], np.cumsum([VS[v] for v in assign])]))
    plan = ctx.eng.skin_plan()
    assert list(plan.perVariant)[:3] == [int((assign == v).sum()) for v in range(3)] and sum(plan.perVariant) == CHARS
    assert plan.totalVertices == off[-1] and plan.capacityVertices == capacity and plan.dropped == 0 and plan.charsPerUnit == 4
    got = ctx.streams(capacity)
    _assert_bits([g[:off[-1]] for g in got], want, "round robin")
    for g in got:
        assert (g[off[-1]:] == SENTINEL).all(), "nothing is written behind the last character"


@pytest.mark.parametrize("cut", ["inside a slice", "on a slice boundary"])
def test_capacity_drops_whole_characters_and_stores_nothing_beyond(world, cut):
    ctx, uniform = world
    assign = np.random.default_rng(7).integers(0, 3, CHARS)
    want, off = _expect_streams(uniform, assign)
    allocated = CHARS * max(VS)
    k = int(np.nonzero(assign[20:] == 0)[0][0]) + 20           # a 1000-vertex character in the back half
    capacity = int(off[k]) + 5 if cut == "inside a slice" else int(off[k + 1])
    fits = off[1:] <= capacity
    assert 0 < fits.sum() < CHARS and fits.sum() == (k if cut == "inside a slice" else k + 1)
    end = int(off[fits.sum()])
    try:
        ctx.eng.reserve_vertices(0)                              # the streams hold CHARS x 1000 vertices from here on
        ctx.eng.reserve_vertices(capacity)
        ctx.fill(allocated)
        ctx.eng.set_mesh_variants(assign)
        ctx.skin()
        plan = ctx.eng.skin_plan()
        assert plan.dropped == CHARS - fits.sum() and plan.capacityVertices == capacity and plan.totalVertices == off[-1]
        assert list(plan.perVariant)[:3] == [int(((assign == v) & fits).sum()) for v in range(3)]
        got = ctx.streams(allocated)
        _assert_bits([g[:end] for g in got], [w[:end] for w in want], "characters that fit")
        for g in got:
            assert (g[end:] == SENTINEL).all(), "dropped characters' slices and everything beyond the capacity are untouched"
        assert np.array_equal(ctx.eng.vertex_offsets(), off), "the offsets say what the crowd asks for"
    finally:
        ctx.eng.reserve_vertices(0)
    ctx.skin()
    assert ctx.eng.skin_plan().dropped == 0
    _assert_bits(ctx.streams(int(off[-1])), want, "after reserve_vertices(0)")


def test_lod_select_matches_a_float64_restatement_and_clamps(world):
    ctx, _ = world
    A = ctx.A
    rng = np.random.default_rng(21)
    eye = np.array([1.25, -3.5, 20.0])
    thresholds = np.array([5.0, 10.0], np.float32)
    pos = eye + rng.normal(0, 8.0, (CHARS, 3))
    d2 = ((pos - eye)[:, 0] ** 2 + (pos - eye)[:, 1] ** 2) + (pos - eye)[:, 2] ** 2
    t2 = thresholds.astype(np.float64) ** 2
    assert (np.abs(d2[:, None] - t2[None]) > 1e-9 * t2[None]).all(), "no seeded body within 1e-9 relative of a threshold"
    bodies = ctx.sge.assets.default_bodies(CHARS, pos)
    ctx.eng.upload(bodies=bodies)
    ctx.eng.lod_select(eye, thresholds)
    vp = C.c_void_p()
    ctx.eng._call("crowd_variant_buffer", C.byref(vp))

    def read_variants():
        ctx.eng.synchronize()
        out = np.empty(CHARS, np.uint8)
        assert _hip().hipMemcpy(out.ctypes.data, vp, CHARS, 2) == 0
        return out

    assert np.array_equal(read_variants(), (d2[:, None] >= t2[None]).sum(1))
    # exact cases, eye at the origin: 25 >= 25 and 100 >= 100
    pos[:3] = [(3, 4, 0), (0, 0, 5), (6, 8, 0)]
    ctx.eng.upload(bodies=ctx.sge.assets.default_bodies(CHARS, pos))
    ctx.eng.lod_select((0.0, 0.0, 0.0), thresholds)
    assert read_variants()[:3].tolist() == [1, 1, 2]
    # more thresholds than uploaded variants: clamped to variant 2
    many = np.array([0.5, 1.0, 2.0, 3.0, 4.0], np.float32)
    ctx.eng.lod_select((0.0, 0.0, 0.0), many)
    d0 = (pos[:, 0] ** 2 + pos[:, 1] ** 2) + pos[:, 2] ** 2
    want = np.minimum((d0[:, None] >= many.astype(np.float64)[None] ** 2).sum(1), 2)
    assert want.max() == 2 and np.array_equal(read_variants(), want)
    # a caller's kernel may write anything: values past the uploaded variants are clamped by the skin launch
    wild = np.full(CHARS, 200, np.uint8)
    assert _hip().hipMemcpy(vp, wild.ctypes.data, CHARS, 1) == 0
    ctx.skin()
    plan = ctx.eng.skin_plan()
    assert list(plan.perVariant)[:3] == [0, 0, CHARS] and plan.totalVertices == CHARS * VS[2]
    ctx.eng.set_mesh_variants(np.zeros(CHARS, np.uint8))
    with pytest.raises(ctx.sge.SgeError):
        ctx.eng.lod_select(eye, [5.0, 5.0])
    with pytest.raises(ctx.sge.SgeError):
        ctx.eng.lod_select(eye, np.arange(8, dtype=np.float32))
    assert A.SGE_MAX_MESH_VARIANTS == 8


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("cpw", [1, 2])
def test_one_and_two_characters_per_unit_are_bit_identical_too(sge, monkeypatch, cpw, layout):
    """skin_variant_kernel<3|4, 1|2>: SGE_SKIN_CPW is read when the context is created. 37 characters leave a partial last group at
    two per unit in every variant that holds an odd number; the six patterns as above, the reported form asserted. (The halving
    loop of variantCharsPerUnit cannot run: two palettes of SGE_MAX_BONES = 256 bones are 24,592 bytes.)"""
    bones = 65
    monkeypatch.delenv("SGE_SKIN_PERSISTENT", raising=False)
    monkeypatch.delenv("SGE_SKIN_CPW", raising=False)
    oracle = _Oracle(sge, bones, layout)
    try:
        uniform = oracle.run(_palettes(bones))
    finally:
        oracle.close()
    monkeypatch.setenv("SGE_SKIN_CPW", str(cpw))
    with _Ctx(sge, bones, layout, [_case(V, bones) for V in VS]) as ctx:
        ctx.write_palettes(_palettes(bones))
        for name, assign in _patterns().items():
            ctx.eng.set_mesh_variants(assign)
            ctx.skin()
            want, off = _expect_streams(uniform, assign)
            assert ctx.form()[1] == cpw and ctx.eng.skin_plan().charsPerUnit == cpw
            _assert_bits(ctx.streams(int(off[-1])), want, "CPW %d %s %s" % (cpw, layout, name))
            assert np.array_equal(ctx.eng.vertex_offsets(), off), name
        assert any((assign == v).sum() % 2 for assign in _patterns().values() for v in range(3))


def test_contract_error_codes(sge):
    A = sge.abi
    bones = 65
    with _Ctx(sge, bones, "packed", [_case(VS[0], bones)], populate=False) as ctx:
        eng, lib = ctx.eng, ctx.eng.t.lib
        rig = _rig(bones)
        eng.upload_skeleton(rig)
        eng.upload_profiles(rig.profiles)

        def variant_upload(v, mesh, inv_bind=None):
            d = A.SkinnedMeshDesc()
            d.vertexCount = mesh["positions"].shape[0]
            keep = {k: np.ascontiguousarray(mesh[k], np.float32) for k in ("positions", "normals", "tangents", "boneWeights")}
            keep["boneIndices"] = np.ascontiguousarray(mesh["boneIndices"], np.uint16)
            for k in ("positions", "normals", "tangents", "boneWeights"):
                setattr(d, k, keep[k].ctypes.data_as(C.POINTER(C.c_float)))
            d.boneIndices = keep["boneIndices"].ctypes.data_as(C.POINTER(C.c_uint16))
            if inv_bind is not None:
                d.invBindModel = inv_bind.ctypes.data_as(C.POINTER(C.c_float))
                d.invBindCount = bones
            return lib.sge_skinned_mesh_variant_upload(eng.h, v, C.byref(d))

        assert variant_upload(1, _case(VS[1], bones)) == A.SGE_ERR_STATE, "before variant 0 exists"
        eng.upload_skinned_mesh(_case(VS[0], bones))
        sge.crowd.spawn_crowd(eng, rig, CHARS, None, mode="lbs")
        # a context that never uploads a variant: no offsets, and the skin stage is the one it always was
        p = C.c_void_p()
        assert lib.sge_crowd_vertex_offsets(eng.h, C.byref(p)) == A.SGE_ERR_STATE
        ctx.skin()
        eng.synchronize()
        assert ctx.form() == (0, 1)
        info = A.SkinPlanInfo()
        assert lib.sge_skin_plan_read(eng.h, C.byref(info)) == A.SGE_ERR_STATE
        # no capacity without a variant: the uniform launch forms write CHARS x V vertices whatever is reserved
        assert lib.sge_crowd_reserve_vertices(eng.h, CHARS) == A.SGE_ERR_STATE and b"variant" in lib.sge_last_error()
        assert lib.sge_crowd_reserve_vertices(eng.h, 0) == A.SGE_OK
        eng.set_option(A.OPT_SKIN_LAYOUT, A.LAYOUT_PADDED16)      # the streams grow with the layout, as they always did
        ctx.skin()
        eng.synchronize()
        p3 = eng.skinned()[0]
        eng.set_option(A.OPT_SKIN_LAYOUT, A.LAYOUT_PACKED)
        ctx.skin()
        p0 = eng.skinned()[0]
        assert p3.shape == p0.shape == (CHARS * VS[0], 3) and np.abs(p3 - p0).max() <= 1e-5 * max(np.abs(p0).max(), 1.0)
        ones = np.ones(CHARS, np.uint8)
        assert lib.sge_characters_set_mesh_variants(eng.h, 0, CHARS, A.ptr(ones)) == A.SGE_ERR_INVALID, "variant 1 was never uploaded"
        assert lib.sge_characters_set_mesh_variants(eng.h, 0, CHARS, A.ptr(np.zeros(CHARS, np.uint8))) == A.SGE_OK
        assert variant_upload(0, _case(VS[1], bones)) == A.SGE_ERR_INVALID, "variant 0 only through sge_skinned_mesh_upload"
        assert variant_upload(8, _case(VS[1], bones)) == A.SGE_ERR_INVALID
        assert variant_upload(1, _case(VS[1], bones), inv_bind=np.zeros((bones, 16), np.float32)) == A.SGE_ERR_INVALID
        bad = dict(_case(VS[1], bones))
        bad["boneIndices"] = bad["boneIndices"].copy()
        bad["boneIndices"][5, 2] = bones
        assert variant_upload(1, bad) == A.SGE_ERR_INVALID, "bone index out of range"
        assert lib.sge_crowd_vertex_offsets(eng.h, C.byref(p)) == A.SGE_ERR_STATE, "a refused upload leaves no variant behind"
        assert variant_upload(1, _case(VS[1], bones)) == A.SGE_OK
        assert lib.sge_characters_set_mesh_variants(eng.h, 0, CHARS, A.ptr(ones)) == A.SGE_OK
        assert lib.sge_characters_set_mesh_variants(eng.h, 0, CHARS, A.ptr(ones * 2)) == A.SGE_ERR_INVALID
        assert lib.sge_crowd_vertex_offsets(eng.h, C.byref(p)) == A.SGE_OK and p.value
        assert lib.sge_crowd_reserve_vertices(eng.h, CHARS - 1) == A.SGE_ERR_INVALID
        # the two refusals while a variant >= 1 exists
        d = A.TickDesc()
        d.dt, d.stages = 0.0, A.STAGE_SKIN | A.STAGE_BLAS_REFIT
        assert lib.sge_tick(eng.h, C.byref(d)) == A.SGE_ERR_STATE and b"variant" in lib.sge_last_error()
        d.stages = A.STAGE_BLAS_REFIT
        assert lib.sge_tick(eng.h, C.byref(d)) == A.SGE_ERR_STATE
        assert lib.sge_blas_refit(eng.h, 0, CHARS) == A.SGE_ERR_STATE and b"variant" in lib.sge_last_error()
        rays, hits = np.zeros(1, A.blas_ray_dtype), np.zeros(1, A.blas_hit_dtype)
        assert lib.sge_blas_intersect_batch(eng.h, A.ptr(rays), 1, A.ptr(hits)) == A.SGE_ERR_STATE and b"variant" in lib.sge_last_error()
        assert lib.sge_blas_intersect_device(eng.h, C.c_void_p(16), 1, C.c_void_p(16), 1) == A.SGE_ERR_STATE and b"variant" in lib.sge_last_error()
        d.stages, d.first, d.count = A.STAGE_SKIN, 3, 10
        assert lib.sge_tick(eng.h, C.byref(d)) == A.SGE_ERR_STATE and b"whole crowd" in lib.sge_last_error()
        d.first, d.count = 0, CHARS
        assert lib.sge_tick(eng.h, C.byref(d)) == A.SGE_OK
        eng.synchronize()
        assert eng.skin_plan().totalVertices == CHARS * VS[1]


# ---- variants change every step under every schedule ---------------------------------------------------------------------------
TICKS = 6


def _scene_ctx(sge, overlap):
    """The small benchmark scene (Y-Bot rig, terrain, 37 characters walking) with the three test meshes."""
    A = sge.abi
    eng = sge.CharacterEngine(0)
    try:
        eng.set_option(A.OPT_PLACEMENT_PROBES, 1)
        eng.set_option(A.OPT_OVERLAP_SKIN, overlap)
        build_scene(sge, eng, CHARS, terrain_cells=(32, 24), seed=3, pose_debug=False)
        eng.upload_skinned_mesh(_case(VS[0], 65))
        for v in (1, 2):
            eng.upload_mesh_variant(v, _case(VS[v], 65))
    except BaseException:
        eng.close()
        raise
    return eng


def _raw(eng, vertices):
    eng.synchronize()
    ptrs = [C.c_void_p() for _ in range(3)]
    eng._call("crowd_buffers", None, *[C.byref(p) for p in ptrs])
    out = [np.empty((vertices, 3), np.float32), np.empty((vertices, 3), np.float32), np.empty((vertices, 4), np.float32)]
    for a, p in zip(out, ptrs):
        assert _hip().hipMemcpy(a.ctypes.data, p, a.nbytes, 2) == 0
    return out


def test_variants_change_every_step_under_every_schedule(sge):
    """Six ticks of the full stage set, a new seeded assignment in front of each. Serial order with a host synchronisation per tick
    gives the palettes and the expected bytes (through the uniform oracle); overlap on the context's own stream and overlap on a
    caller's stream run the same six ticks WITHOUT a host synchronisation in the loop, a consumer stream ordering itself with
    sge_skin_wait / sge_skin_consumed and copying streams and offsets device to device. The assignment for tick n + 1 is enqueued
    while skin(n) may still be in flight: its plan must not see it, and skin(n + 1) must."""
    import torch
    A = sge.abi
    rng = np.random.default_rng(3)
    assigns = [rng.integers(0, 3, CHARS) for _ in range(TICKS)]
    assert all(len(set(a.tolist())) == 3 for a in assigns) and any((a != b).any() for a, b in zip(assigns, assigns[1:]))
    capacity = CHARS * max(VS)

    eng = _scene_ctx(sge, 0)
    serial, pals = [], []
    try:
        for a in assigns:
            eng.set_mesh_variants(a)
            eng.tick()
            pals.append(eng.palettes()[0])
            serial.append((_raw(eng, capacity), eng.vertex_offsets()))
    finally:
        eng.close()
    assert np.abs(pals[0] - pals[-1]).max() > 1e-3, "the pose moves over the six ticks"

    oracle = _Oracle(sge, 65, "packed")
    try:
        for t, a in enumerate(assigns):
            want, off = _expect_streams(oracle.run(pals[t]), a)
            got, goff = serial[t]
            assert np.array_equal(goff, off), t
            _assert_bits([g[:off[-1]] for g in got], want, "serial tick %d" % t)
    finally:
        oracle.close()

    hip = _hip()
    dev = torch.device("cuda", 0)
    for overlap, own_stream in ((1, True), (2, False)):
        eng = _scene_ctx(sge, overlap)
        lib, h = eng.t.lib, eng.h
        try:
            consumer = torch.cuda.Stream(device=0)
            caller = None
            if not own_stream:
                caller = torch.cuda.Stream(device=0)
                assert lib.sge_context_set_stream(h, C.c_void_p(caller.cuda_stream)) == 0
            ptrs = [C.c_void_p() for _ in range(3)]
            eng._call("crowd_buffers", None, *[C.byref(p) for p in ptrs])
            offp = C.c_void_p()
            eng._call("crowd_vertex_offsets", C.byref(offp))
            copies = []
            for a in assigns:
                eng.set_mesh_variants(a)
                eng.tick()
                assert lib.sge_skin_wait(h, C.c_void_p(consumer.cuda_stream)) == 0
                bufs = [torch.empty((capacity, 3), dtype=torch.float32, device=dev), torch.empty((capacity, 3), dtype=torch.float32, device=dev),
                        torch.empty((capacity, 4), dtype=torch.float32, device=dev), torch.empty(CHARS + 1, dtype=torch.int64, device=dev)]
                for b, p in zip(bufs, ptrs + [offp]):
                    assert hip.hipMemcpyAsync(C.c_void_p(b.data_ptr()), p, b.numel() * b.element_size(), 3, C.c_void_p(consumer.cuda_stream)) == 0
                assert lib.sge_skin_consumed(h, C.c_void_p(consumer.cuda_stream)) == 0
                copies.append(bufs)
            eng.synchronize()
            consumer.synchronize()
            form = C.c_int32(-1), C.c_int32(-1)
            assert lib.sge_debug_skin_form(h, C.byref(form[0]), C.byref(form[1])) == 0 and form[1].value == 4
            for t, bufs in enumerate(copies):
                got, goff = [b.cpu().numpy() for b in bufs[:3]], bufs[3].cpu().numpy()
                want, woff = serial[t]
                assert np.array_equal(goff, woff), (overlap, t)
                _assert_bits([g[:woff[-1]] for g in got], [w[:woff[-1]] for w in want], "overlap %d tick %d" % (overlap, t))
            if caller is not None:
                assert lib.sge_context_set_stream(h, None) == 0
        finally:
            eng.close()


@pytest.mark.parametrize("overlap,own_stream", [(1, True), (2, False)])
def test_a_write_behind_the_tick_does_not_reach_a_launch_still_queued(sge, overlap, own_stream):
    """The host far ahead of the device: a consumer stream is kept busy for a few milliseconds and handed to sge_skin_consumed, so
    the context's streams wait for it while the host enqueues set(A) tick set(B) tick set(C) tick set(D) with nothing in between.
    The main stream runs its copies of the variant bytes and the later writes long before the skin stream reaches the plan kernels
    (each waits for its tick's pose launch): a plan that read the live array, or a third copy that overwrote the slot of the
    first under its plan, would not leave tick three with assignment C. The result must be C's bytes and offsets, not D's."""
    import torch
    A = sge.abi
    rng = np.random.default_rng(11)
    a_, b_, c_, d_ = [rng.integers(0, 3, CHARS) for _ in range(4)]
    assert (c_ != d_).any() and (c_ != a_).any() and (c_ != b_).any()
    eng = _scene_ctx(sge, overlap)
    lib, h = eng.t.lib, eng.h
    try:
        consumer = torch.cuda.Stream(device=0)
        caller = None
        if not own_stream:
            caller = torch.cuda.Stream(device=0)
            assert lib.sge_context_set_stream(h, C.c_void_p(caller.cuda_stream)) == 0
        eng.set_mesh_variants(a_)
        eng.tick()                       # code objects loaded, both palette buffers written once
        eng.tick()
        eng.synchronize()
        with torch.cuda.stream(consumer):
            torch.cuda._sleep(4_000_000)
        assert lib.sge_skin_consumed(h, C.c_void_p(consumer.cuda_stream)) == 0
        for assign in (a_, b_, c_):
            eng.set_mesh_variants(assign)
            eng.tick()
        eng.set_mesh_variants(d_)
        eng.synchronize()
        consumer.synchronize()
        plan = eng.skin_plan()
        assert list(plan.perVariant)[:3] == [int((c_ == v).sum()) for v in range(3)]
        pal = eng.palettes()[0]
        got, goff = _raw(eng, CHARS * max(VS)), eng.vertex_offsets()
        if caller is not None:
            assert lib.sge_context_set_stream(h, None) == 0
    finally:
        eng.close()
    oracle = _Oracle(sge, 65, "packed")
    try:
        want, off = _expect_streams(oracle.run(pal), c_)
    finally:
        oracle.close()
    assert np.array_equal(goff, off)
    _assert_bits([g[:off[-1]] for g in got], want, "tick three of three, overlap %d" % overlap)
