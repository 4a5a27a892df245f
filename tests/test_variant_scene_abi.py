"""CPU tests of the additions for a crowd with mesh variants in the ray scene (include/sge_amd_variant_scene.h): the new header, its
ctypes mirror and the library agree; the older headers and their mirrors are what they were; the three ragged kernels use no
scratch, spill nothing and stay inside 128 registers, and the uniform kernels are still counted as before. (A context cannot be
created without a GPU, so the contract itself is tested in test_gpu_variant_scene.py.)"""
import ctypes as C
import importlib.util
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "sge_amd_variant_scene.h")
OLDER = {"sge_amd.h": "PROTOTYPES", "sge_amd_variants.h": "VARIANT_PROTOTYPES", "sge_amd_variant_blas.h": "VARIANT_BLAS_PROTOTYPES",
         "sge_amd_ray_scene.h": "SCENE_PROTOTYPES", "sge_amd_render.h": "RENDER_PROTOTYPES"}
COUNTS = {"sge_amd_variants.h": 7, "sge_amd_variant_blas.h": 6, "sge_amd_ray_scene.h": 10, "sge_amd_render.h": 6}
RAGGED = ("scene_ragged_trace_kernel", "scene_ragged_occlusion_kernel", "render_ragged_frame_kernel")
COUNTED = (("scene_trace_kernel", 2), ("scene_occlusion_kernel", 2), ("scene_instance_boxes_kernel", 1), ("render_frame_kernel", 2))
# every fragment an older test counts kernels by
OTHER = ("skin_kernel", "pose_kernel", "move_kernel", "move_group_kernel", "skin_ticket", "blas_refit_kernel", "blas_intersect_kernel",
         "blas_world_boxes_kernel", "blas_refit_ragged_kernel", "blas_intersect_ragged_kernel", "blas_world_boxes_ragged_kernel",
         "skin_variant_kernel", "variant_plan_kernel", "lod_select_kernel")


@pytest.fixture(scope="module")
def lib(sge):
    import __graft_entry__
    __graft_entry__.build()
    return sge.abi.load_library()


def declared_functions(path):
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(sge_[a-z0-9_]+)\s*\(", text)))


def test_header_mirror_and_exports_agree(sge, lib):
    names = declared_functions(HEADER)
    assert names == ["sge_scene_crowd_status_get"] == sorted(sge.abi.VARIANT_SCENE_PROTOTYPES)
    out = subprocess.check_output(["nm", "-D", "--defined-only", sge.abi.library_path()], text=True)
    assert set(names) <= {l.split()[-1] for l in out.splitlines() if " T " in l}
    for name in names:
        assert getattr(lib, name).argtypes == sge.abi.VARIANT_SCENE_PROTOTYPES[name][1], name
    text = open(HEADER).read()
    assert re.search(r"#define SGE_HAS_VARIANT_SCENE 1\b", text)
    assert '#include "sge_amd_variant_blas.h"' in text and '#include "sge_amd_render.h"' in text
    for k, word in enumerate(("OK", "NO_MESH", "NO_STRUCTURE", "NO_CHARACTERS", "VARIANT_NOT_BUILT", "NO_BUFFERS")):
        assert re.search(r"#define SGE_SCENE_CROWD_%s %d\b" % (word, k), text) and getattr(sge.abi, "SCENE_CROWD_" + word) == k
    assert hasattr(sge.CharacterEngine, "scene_crowd_status")
    host = open(os.path.join(ROOT, "swift-game-engine_amd", "host", "sge_host.hpp")).read()
    assert "sge_scene_crowd_status_get" in host and "sge_amd_variant_scene.h" in host


def test_the_struct_matches_the_header(sge, tmp_path):
    st = sge.abi.SceneCrowdStatus
    lines = ['printf("%zu", sizeof(struct sge_scene_crowd_status));']
    for field, _t in st._fields_:
        lines.append('printf(" %%zu", offsetof(struct sge_scene_crowd_status, %s));' % field)
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sge_amd_variant_scene.h"\nint main(void){%s return 0;}\n' % "".join(lines))
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-I", INCLUDE, str(src), "-o", str(exe)])
    row = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert [f for f, _ in st._fields_] == ["crowdReady", "ragged", "reason", "variant"]
    assert row[0] == 16 == C.sizeof(st) and row[1:] == [getattr(st, f).offset for f, _ in st._fields_] == [0, 4, 8, 12]


def test_the_older_headers_keep_their_prototypes(sge, lib):
    new = set(sge.abi.VARIANT_SCENE_PROTOTYPES)
    for header, table in OLDER.items():
        path = os.path.join(INCLUDE, header)
        protos = getattr(sge.abi, table)
        assert declared_functions(path) == sorted(protos), header
        assert header not in COUNTS or len(protos) == COUNTS[header]
        assert not new & set(protos)
    for header in ("sge_amd_ray_scene.h", "sge_amd_render.h"):  # no longer say that variants and the scene exclude each other
        text = open(os.path.join(INCLUDE, header)).read()
        assert "not implemented" not in text and "mesh variants included" not in text and "sge_amd_variant_scene.h" in text
    assert lib.sge_abi_version() == 2 and re.search(r"#define SGE_ABI_VERSION 2\b", open(os.path.join(INCLUDE, "sge_amd.h")).read())


def test_the_ragged_kernels_spill_nothing_and_the_uniform_ones_are_counted_as_before(sge, lib):
    """Two instances (stride 3 and 4) of each ragged kernel: no scratch, no VGPR or SGPR spills, no dynamic stack, at most 128 VGPRs;
    none of their names contains a fragment an older test counts. The counted uniform kernels are still 2 / 2 / 1 / 2."""
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    tab = kr.kernel_table(sge.abi.library_path())
    for frag in RAGGED:
        hits = {k: v for k, v in tab.items() if frag in k}
        assert len(hits) == 2, (frag, sorted(hits))
        for name, r in hits.items():
            print(name, r)
            assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and not r["dynamic_stack"], (name, r)
            assert r["vgpr"] <= 128, (name, r)
            for other in OTHER + tuple(f for f, _ in COUNTED):
                assert other not in name, (name, other)
    for frag, count in COUNTED:
        hits = {k: v for k, v in tab.items() if frag in k}
        assert len(hits) == count, (frag, sorted(hits))
        for name, r in hits.items():
            assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and not r["dynamic_stack"] and r["vgpr"] <= 128, (name, r)


def test_a_null_context_is_refused(sge, lib):
    st = sge.abi.SceneCrowdStatus(7, 7, 7, 7)
    assert lib.sge_scene_crowd_status_get(None, C.byref(st)) == sge.abi.SGE_ERR_INVALID
    assert (st.crowdReady, st.ragged, st.reason, st.variant) == (7, 7, 7, 7) and b"bad argument" in lib.sge_last_error()
