"""Every launch form of the linear-blend skinning (csrc/sge_skin.hip) against the float64 reference of tests/skin_ref.py, per
element, at the shapes where the forms' copies of the arithmetic and their index arithmetic can go wrong:

    plain                         skin_kernel<3, 3|4>                      overlap off
    resident, one character       skin_ticket_kernel<3, 3|4>               overlap on, SGE_SKIN_PERSISTENT=1, < 64 characters or CPW 1
    resident, CPW characters      skin_ticket_multi_kernel<3|4, 2|4|8>     overlap on, resident, >= 64 characters
    job list                      skin_jobs_kernel<3|4>, source stride 3|4 sge_skinning_encode with more than one job
    fused with the refit          skin_refit_kernel<3, 3|4, TILE>          SGE_STAGE_SKIN | SGE_STAGE_BLAS_REFIT, overlap off

The palettes are the pose stage's own (a random rig, a mixed crowd ticked a few steps), read back and fed to the reference, so the
bars (skin_ref's docstring: 9 u mag for positions, 9 u ||magN|| / ||N|| + 6 u for directions, u = 2**-24) see the skinning kernel
alone. Every case asserts which form ran (sge_debug_skin_form) and checks all chars * V vertices of the three streams, read raw
from the device so that the padding float of the padded16 layout is seen too.

`palettes()` copies dPalettes[palRead]; a skin stage without a pose stage reads crowd.palettes, which the newest pose stage set
to that very buffer (sge_tick), also in overlap mode where the palettes alternate between two buffers: the read-back is what the
newest skin launch read.

The skinned output streams are allocated to exactly chars * V vertices (allocCrowdOutputs): there is no room past the crowd's
last character for a canary. What a partial last group could overrun is checked where room exists: the sub-range test ends its
range on a partial group in the middle of the crowd and requires the characters behind it to be untouched.

`-s` shows a line `skin-forms <case> position <ratio> direction <ratio>` per case: the worst error as a fraction of the bar."""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle_binding as ob
from blas_ref import expected_bounds
from scenes import _SyntheticRig, assert_close
from skin_ref import check_streams, make_skin_case, skin_reference

pytestmark = pytest.mark.gpu

BONES = 33          # the crowd cases' rig: one pass of the pose kernel, cheap to tick
LAYOUTS = ["packed", "padded16"]
BLOCK = 256         # kSkinBlock


@functools.lru_cache(maxsize=None)
def _rig(bones):
    return _SyntheticRig(bones, 4, seed=500 + bones, animate_all=True, translate_some=True)


@functools.lru_cache(maxsize=None)
def _case(V, B):
    """Shared between the tests and never written to."""
    case = make_skin_case(V, B, seed=1000 * B + V)
    for a in case.values():
        a.setflags(write=False)
    return case


def _splits(units, V):
    """launch_skin's rule for `units` characters (or groups of CPW characters) of V vertices -> (splits, vertsPerSplit)."""
    s = 1
    while units * s < 8192 and s < 64 and (V + s - 1) // s > 2 * BLOCK:
        s *= 2
    vps = ((V + s - 1) // s + BLOCK - 1) // BLOCK * BLOCK
    return (V + vps - 1) // vps, vps


def _resident_workgroups(quarters=1):
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count * quarters // 4


def _pose_stages(A):
    return A.STAGE_LOCOMOTION | A.STAGE_ACTION | A.STAGE_POSE | A.STAGE_WRITEBACK


def _populate(sge, eng, rig, case, chars):
    """Skeleton, profiles, the case's mesh and a crowd in "lbs" mode whose clones are spread over the four locomotion states,
    some mid-blend, each at its own phase (the same state for every engine it is called on)."""
    A = sge.abi
    eng.upload_skeleton(rig)
    eng.upload_profiles(rig.profiles)
    eng.upload_skinned_mesh(case)
    st = sge.crowd.spawn_crowd(eng, rig, chars, None, mode="lbs")
    rng = np.random.default_rng(77)
    loco = st["locomotion"].copy()
    loco["state"] = np.arange(chars) % 4
    loco["fromState"] = (np.arange(chars) // 4) % 4
    blending = rng.uniform(size=chars) < 0.25
    loco["flags"] |= np.where(blending, A.LOCO_IS_BLENDING, 0).astype(np.uint32)
    loco["blendT"] = np.where(blending, rng.uniform(0, 1, chars), 1.0)
    for s in range(4):
        loco["time"][:, s] = rng.uniform(0, rig.profiles[int(loco["profile"][0, s])]["cycleDuration"], chars)
    eng.upload(locomotion=loco)


class _Crowd:
    """A fresh context per case: SGE_SKIN_PERSISTENT / SGE_SKIN_CPW are read when the context is created."""

    def __init__(self, sge, monkeypatch, chars, V, layout, overlap, persistent=None, cpw=None, bones=BONES, pose_steps=3):
        A = sge.abi
        for name, value in (("SGE_SKIN_PERSISTENT", persistent), ("SGE_SKIN_CPW", cpw)):
            if value is None:
                monkeypatch.delenv(name, raising=False)
            else:
                monkeypatch.setenv(name, str(value))
        self.sge, self.A, self.chars, self.V, self.bones = sge, A, chars, V, bones
        self.stride = 4 if layout == "padded16" else 3
        self.case = _case(V, bones)
        self.rig = _rig(bones)
        self.gpu = sge.CharacterEngine(0)
        try:
            self.gpu.set_option(A.OPT_PLACEMENT_PROBES, 1)
            self.gpu.set_option(A.OPT_SKIN_LAYOUT, A.LAYOUT_PADDED16 if layout == "padded16" else A.LAYOUT_PACKED)
            self.gpu.set_option(A.OPT_OVERLAP_SKIN, 1 if overlap else 0)
            _populate(sge, self.gpu, self.rig, self.case, chars)
            self.pose(pose_steps)
        except BaseException:
            self.gpu.close()
            raise

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.gpu.close()

    def pose(self, steps):
        for _ in range(steps):
            self.gpu.tick(stages=_pose_stages(self.A))

    def skin(self, first=0, count=0, extra=0):
        self.gpu.tick(dt=0.0, stages=self.A.STAGE_SKIN | extra, first=first, count=count)
        self.gpu.synchronize()

    def form(self):
        q, cpw = C.c_int32(-1), C.c_int32(-1)
        assert self.gpu.t.lib.sge_debug_skin_form(self.gpu.h, C.byref(q), C.byref(cpw)) == 0
        return q.value, cpw.value

    def streams(self):
        """The three output streams as they lie in device memory: [chars * V][3 or 4], same, [chars * V][4]."""
        self.gpu.synchronize()
        hip = C.CDLL("libamdhip64.so")
        hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        ptrs = [C.c_void_p() for _ in range(3)]
        self.gpu._call("crowd_buffers", None, *[C.byref(p) for p in ptrs])
        n = self.chars * self.V
        out = [np.empty((n, self.stride), np.float32), np.empty((n, self.stride), np.float32), np.empty((n, 4), np.float32)]
        for a, p in zip(out, ptrs):
            assert p.value and hip.hipMemcpy(a.ctypes.data, p, a.nbytes, 2) == 0  # hipMemcpyDeviceToHost
        return out

    def check(self, name, palettes=None):
        """Every vertex of the crowd against the reference over the palettes the skin launch read."""
        pal = self.gpu.palettes()[0] if palettes is None else palettes
        assert np.abs(pal[0] - pal[-1]).max() > 1e-3 or self.chars == 1, "the clones have palettes of their own"
        ref = skin_reference(self.case, pal)
        got = self.streams()
        rp, rd = check_streams(*got, ref, name)
        print("skin-forms %s position %.3f direction %.3f" % (name, rp, rd))
        return got


# ---- plain form -----------------------------------------------------------------------------------------------------------
# launch_skin: splits doubles while chars * splits < 8192, splits < 64 and ceil(V / splits) > 512; vertsPerSplit is
# ceil(V / splits) rounded up to 256 and splits = ceil(V / vertsPerSplit):
#   V = 1, 255, 256, 257   one split (of 256 / 256 / 256 / 512 vertices); 257 is one chunk of 256 and one of a single vertex
#   V = 513                1 -> 2 (513 > 512), stop (257); vertsPerSplit 512, two splits, the last of 1 vertex
#   V = 1300               1 -> 2 -> 4 (650 > 512), stop (325); vertsPerSplit 512, three splits of 512, 512 and 276 vertices
PLAIN_SHAPES = [(1, 1), (3, 255), (3, 256), (3, 257), (2, 1300), (70, 513)]


def test_plain_shapes_reach_a_short_last_split():
    assert _splits(2, 1300) == (3, 512) and 1300 % 512 != 0
    assert _splits(70, 513) == (2, 512) and _splits(3, 257) == (1, 512) and _splits(3, 256) == (1, 256)
    assert any(_splits(c, v)[0] > 1 and v % _splits(c, v)[1] != 0 for c, v in PLAIN_SHAPES)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("chars,V", PLAIN_SHAPES)
def test_plain_form(sge, monkeypatch, chars, V, layout):
    with _Crowd(sge, monkeypatch, chars, V, layout, overlap=False) as cw:
        cw.skin()
        assert cw.form() == (0, 1)
        cw.check("plain %dx%d %s" % (chars, V, layout))


# ---- resident, one character per unit ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("chars,V,cpw", [(37, 513, None), (131, 1300, 1)])
def test_resident_one_character_form(sge, monkeypatch, chars, V, cpw, layout):
    """skin_ticket_kernel: 37 characters lie below the 64-character gate of the multi-character form, 131 take it through
    SGE_SKIN_CPW=1. More units than resident workgroups (a quarter of a workgroup per CU), so the later units are drawn from the
    ticket counter; three launches in a row, each checked: the counter has to be back at zero for the next (ticketsDone)."""
    units = chars * _splits(chars, V)[0]
    assert units > _resident_workgroups(), (units, _resident_workgroups())
    with _Crowd(sge, monkeypatch, chars, V, layout, overlap=True, persistent=1, cpw=cpw) as cw:
        for run in range(3):
            cw.skin()
            assert cw.form() == (1, 1)
            cw.check("resident-1 %dx%d %s run %d" % (chars, V, layout, run))
            cw.pose(1)


# ---- resident, CPW characters per unit ----------------------------------------------------------------------------------------
def _multi_cases():
    cases = []
    for cpw in (2, 4, 8):
        for layout in LAYOUTS:
            for chars in sorted({64, 65, 64 + cpw - 1} | ({131} if cpw < 8 else set())):
                cases.append((cpw, layout, chars, 513))
    cases.append((4, "packed", 131, 1300))
    cases.append((8, "packed", 267, 513))   # CPW 8 with more units than resident workgroups: 34 groups x 2 splits
    return cases


def test_multi_cases_reach_partial_groups_and_the_ticket_counter():
    cases = _multi_cases()
    for cpw in (2, 4, 8):
        mine = [c for c in cases if c[0] == cpw]
        assert any(c[2] % cpw for c in mine) and any(c[2] % cpw == 0 for c in mine)
        assert any(c[2] % cpw == cpw - 1 for c in mine) and any(c[2] % cpw == 1 for c in mine)
        # 64 resident workgroups on the 256 compute units of the MI355X (the GPU test asserts it from the device's own count)
        assert any(-(-c[2] // cpw) * _splits(-(-c[2] // cpw), c[3])[0] > 64 for c in mine)


@pytest.mark.parametrize("cpw,layout,chars,V", _multi_cases())
def test_resident_multi_character_form(sge, monkeypatch, cpw, layout, chars, V):
    """skin_ticket_multi_kernel<3|4, 2|4|8>: full groups only (64), a last group of one character (65), a last group one short
    (64 + CPW - 1), and crowds whose units exceed the resident workgroups. The characters of a partial last group are checked like
    every other."""
    groups = -(-chars // cpw)
    units = groups * _splits(groups, V)[0]
    if (cpw, chars) in ((2, 131), (4, 131), (8, 267)):
        assert units > _resident_workgroups(), (units, _resident_workgroups())
    with _Crowd(sge, monkeypatch, chars, V, layout, overlap=True, persistent=1, cpw=cpw) as cw:
        for run in range(2):
            cw.skin()
            assert cw.form() == (1, cpw)
            cw.check("resident-%d %dx%d %s run %d" % (cpw, chars, V, layout, run))
            cw.pose(1)


# ---- fewer characters per unit for rigs with many bones -------------------------------------------------------------------------
@pytest.mark.parametrize("bones,expect", [(170, 8), (171, 4), (256, 4)])
def test_characters_per_unit_halve_when_the_palettes_pass_64_kib(sge, monkeypatch, bones, expect):
    """CPW palettes of 48 bytes per bone + 16 bytes have to fit the 64 KiB a kernel may ask for: 8 x 170 x 48 + 16 = 65,296 fits,
    8 x 171 x 48 + 16 = 65,680 does not and the launch takes 4 characters per unit. Bone indices reach B - 1 (make_skin_case).
    At 256 bones (SGE_MAX_BONES) the pose kernel's palettes are compared with the oracle's as well."""
    chars, V = 64, 257
    with _Crowd(sge, monkeypatch, chars, V, "packed", overlap=True, persistent=1, cpw=8, bones=bones) as cw:
        assert int(cw.case["boneIndices"].max()) == bones - 1
        cw.skin()
        assert cw.form() == (1, expect)
        cw.check("resident-8->%d %d bones %dx%d" % (expect, bones, chars, V))
        if bones == 256:
            cpu = ob.oracle_engine()
            try:
                _populate(sge, cpu, cw.rig, cw.case, chars)
                for _ in range(3):
                    cpu.tick(stages=_pose_stages(sge.abi))
                assert_close(cw.gpu.palettes()[0], cpu.palettes()[0], "palette of the 256-bone rig", group=bones * 16)
            finally:
                cpu.close()


# ---- a sub-range of the crowd --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["resident-4", "plain"])
def test_sub_range_skin_stage(sge, monkeypatch, form):
    """sge_tick with first = 5, count = 66 of 80 characters: the palette base and dstBaseVertex are offset, the resident form's
    last group holds 2 of 4 characters. Characters 5..70 carry the new pose, the others keep every bit of the first launch —
    characters 71..79 lie right behind the partial group's slice of the streams."""
    chars, V, first, count = 80, 513, 5, 66
    resident = form == "resident-4"
    assert count % 4 == 2
    with _Crowd(sge, monkeypatch, chars, V, "packed", overlap=resident, persistent=1 if resident else None, cpw=4 if resident else None) as cw:
        want_form = (1, 4) if resident else (0, 1)
        cw.skin()
        assert cw.form() == want_form
        before = cw.check("%s whole crowd before the sub-range" % form)
        cw.pose(2)
        cw.skin(first=first, count=count)
        assert cw.form() == want_form
        pal = cw.gpu.palettes()[0]
        after = cw.streams()
        inside = slice(first * V, (first + count) * V)
        ref = skin_reference(cw.case, pal[first:first + count])
        rp, rd = check_streams(*[a[inside] for a in after], ref, "%s sub-range" % form)
        print("skin-forms %s sub-range position %.3f direction %.3f" % (form, rp, rd))
        assert np.abs(after[0][inside] - before[0][inside]).max() > 1e-3, "the pose moved between the two launches"
        for a, b in zip(after, before):
            assert np.array_equal(a[:first * V].view(np.uint32), b[:first * V].view(np.uint32))
            assert np.array_equal(a[(first + count) * V:].view(np.uint32), b[(first + count) * V:].view(np.uint32))


# ---- job list ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
def test_job_list_form(sge, layout):
    """sge_skinning_encode over several jobs is one launch of skin_jobs_kernel (sge_api.hip takes that path for every list of more
    than one job; the plain kernel serves a single job): the vertex and bone counts and the mixed source strides of
    test_skinning_encode_job_list, here against the float64 bars. 7.0 stays in the gaps between the jobs."""
    import torch
    from skin_ref import rigid_shear_palette

    A = sge.abi
    counts = [1, 255, 256, 257, 5000, 33]
    bones = [3, 65, 17, 256, 65, 1]
    padded_src = [False, True, False, False, True, False]
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(12)
    base, total = [], 0
    for v in counts:
        total += int(rng.integers(1, 5))            # gaps between the jobs' destination ranges
        base.append(total)
        total += v
    total += 3
    jobs, keep, refs = [], [], []
    for v, b, pad, b0 in zip(counts, bones, padded_src, base):
        case = _case(v, b)
        pal = rigid_shear_palette(b, rng, translation=30.0)
        refs.append(skin_reference(case, pal))
        on_dev = {}
        for k, name in (("positions", "sourcePositions"), ("normals", "sourceNormals"), ("tangents", "sourceTangents"),
                        ("boneIndices", "sourceBoneIndices"), ("boneWeights", "sourceBoneWeights")):
            src = np.array(case[k])
            if pad and k in ("positions", "normals"):
                src = np.zeros((v, 4), np.float32)
                src[:, :3] = case[k]
            on_dev[name] = torch.from_numpy(np.ascontiguousarray(src)).to(dev)
        on_dev["palette"] = torch.from_numpy(pal).to(dev)
        keep.append(on_dev)
        jobs.append(dict({k: t.data_ptr() for k, t in on_dev.items()}, paletteCount=b, vertexCount=v, dstBaseVertex=b0,
                         sourceLayout=A.LAYOUT_PADDED16 if pad else A.LAYOUT_PACKED))
    stride = 4 if layout == "padded16" else 3
    gpu = sge.CharacterEngine(0)
    try:
        out = [torch.full((total, stride), 7.0, dtype=torch.float32, device=dev), torch.full((total, stride), 7.0, dtype=torch.float32, device=dev),
               torch.full((total, 4), 7.0, dtype=torch.float32, device=dev)]
        torch.cuda.synchronize()
        gpu.skinning_encode(out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), A.LAYOUT_PADDED16 if layout == "padded16" else A.LAYOUT_PACKED, jobs)
        gpu.synchronize()
        got = [o.cpu().numpy() for o in out]
    finally:
        gpu.close()
    gaps = np.ones(total, bool)
    worst = [0.0, 0.0]
    for v, b, b0, ref in zip(counts, bones, base, refs):
        gaps[b0:b0 + v] = False
        rp, rd = check_streams(*[g[b0:b0 + v] for g in got], ref, "job %d vertices %d bones %s" % (v, b, layout))
        worst = [max(worst[0], rp), max(worst[1], rd)]
    print("skin-forms job-list %s position %.3f direction %.3f" % (layout, *worst))
    assert gaps.sum() >= len(counts) + 3
    for g in got:
        assert (g[gaps] == 7.0).all(), "nothing is written between the jobs"


# ---- fused with the refit --------------------------------------------------------------------------------------------------------
def _strip(V):
    """Triangles (i, i + 1, i + 2) over consecutive vertices, every second one turned: every vertex is referenced, the last too."""
    i = np.arange(V - 2, dtype=np.uint32)
    t = np.stack([i, i + 1, i + 2], 1)
    t[1::2] = t[1::2][:, [1, 0, 2]]
    return t.reshape(-1)


def _refit_tiles(info, V):
    """HostBlas::build's tile rule (sge_host.cpp; LDS sizes from sge_internal.hpp) -> (tile cap, vertices per tile, tiles, vertices
    in the last tile): the largest cap of 4096 / 3072 / 2048 of which three workgroups' LDS fits a CU's 160 KiB (4096 if none does);
    the tiles are balanced and a multiple of 64 vertices long."""
    topo = (info.levels + 2 * info.wideCount + 2) * 4 + 16
    cap = 4096
    for c in (4096, 3072, 2048):
        if 3 * ((info.entryCount + 1) * 24 + c * 12 + (V // c + 2 + 1) * 4 + topo + 256) <= 160 * 1024:
            cap = c
            break
    tiles = (V + cap - 1) // cap
    per = ((V + tiles - 1) // tiles + 63) // 64 * 64
    tiles = (V + per - 1) // per
    return cap, per, tiles, V - (tiles - 1) * per


# V = 700: a single tile (of 704 vertices' room). V = 65,537: 33 tiles of 2,048, the last holding 1 vertex. V = 55,553: 28 tiles
# of 2,048, the last holding 257 vertices. (Balanced tiles leave a last tile that short only when every other tile is full.)
FUSED_SHAPES = [(3, 700, (1, 700)), (70, 700, (1, 700)), (3, 65537, (33, 1)), (3, 55553, (28, 257))]


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("chars,V,tiles", FUSED_SHAPES)
def test_fused_skin_and_refit_form(sge, monkeypatch, chars, V, tiles, layout):
    """skin_refit_kernel (blendAndTransform is a third text of the arithmetic): the streams meet the bars, the boxes are the exact
    min / max of the float32 positions the kernel stored. Which kernel ran: with SGE_OPT_PROFILE on, the two-launch path brackets a
    refit launch of its own and the fused path brackets none."""
    A = sge.abi
    with _Crowd(sge, monkeypatch, chars, V, layout, overlap=False) as cw:
        gpu = cw.gpu
        indices = _strip(V)
        topo = sge.CharacterEngine.blas_topology(cw.case["positions"], indices)
        assert _refit_tiles(topo["info"], V)[2:] == tiles
        gpu.blas_build(indices)
        gpu.set_option(A.OPT_PROFILE, 1)
        gpu.set_option(A.OPT_FUSE_BLAS_REFIT, 0)
        cw.skin(extra=A.STAGE_BLAS_REFIT)
        assert gpu.blas_profile()[1] == 1, "the two-launch path has a refit launch"
        two_launch_boxes = gpu.blas_bounds()
        cw.pose(1)
        gpu.set_option(A.OPT_FUSE_BLAS_REFIT, 1)
        gpu.profile_read(reset=True)
        cw.skin(extra=A.STAGE_BLAS_REFIT)
        assert gpu.blas_profile()[1] == 0 and gpu.profile_read().skin_launches == 1, "one launch: the fused kernel"
        got = cw.check("fused %dx%d %s" % (chars, V, layout))
        boxes = gpu.blas_bounds()
        assert not np.array_equal(boxes, two_launch_boxes), "the pose moved between the two ticks"
        pos = np.ascontiguousarray(got[0][:, :3])
        for c in range(chars):
            want = expected_bounds(topo, indices, pos[c * V:(c + 1) * V])
            assert np.array_equal(boxes[c], want), (c, np.argwhere(boxes[c] != want)[:4])


# ---- the forms against each other --------------------------------------------------------------------------------------------------
def test_resident_forms_write_identical_streams(sge, monkeypatch):
    """skinRangeMulti's comment claims the streams of the one-character form bit for bit: 67 characters x 1,300 vertices (three
    splits, the last short; a partial last group for every CPW) through skin_ticket_kernel and skin_ticket_multi_kernel<3, 2|4|8>
    on the same palettes. The plain form is another instantiation: what test_skinning_kernel_vs_oracle allows between those."""
    chars, V = 67, 1300
    outs, pals = {}, {}
    for name, kw, want in (("plain", dict(overlap=False), (0, 1)), ("resident-1", dict(overlap=True, persistent=1, cpw=1), (1, 1)),
                           ("resident-2", dict(overlap=True, persistent=1, cpw=2), (1, 2)), ("resident-4", dict(overlap=True, persistent=1, cpw=4), (1, 4)),
                           ("resident-8", dict(overlap=True, persistent=1, cpw=8), (1, 8))):
        with _Crowd(sge, monkeypatch, chars, V, "packed", **kw) as cw:
            cw.skin()
            assert cw.form() == want
            outs[name], pals[name] = cw.streams(), cw.gpu.palettes()[0]
    for name in outs:
        assert np.array_equal(pals[name].view(np.uint32), pals["plain"].view(np.uint32)), "the pose stage gives every context the same palettes"
    for name in ("resident-2", "resident-4", "resident-8"):
        for a, b, what in zip(outs[name], outs["resident-1"], ("positions", "normals", "tangents")):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (name, what, np.argwhere(a != b)[:4])
    p, n, t = outs["plain"]
    q = outs["resident-1"]
    assert np.abs(p - q[0]).max() <= 1e-6 * np.abs(p).max() and np.abs(n - q[1]).max() <= 3e-7 and np.abs(t - q[2]).max() <= 3e-7
