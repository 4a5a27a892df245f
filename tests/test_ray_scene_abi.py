"""CPU tests of the ray scene's additions to the C ABI (include/sge_amd_ray_scene.h): the new header, its ctypes mirror and the
library agree; the older headers and their mirrors are what they were; the new kernels use no scratch, spill nothing and stay
inside 128 registers. (A context cannot be created without a GPU, so the host-side validation is tested in
test_gpu_ray_scene.py.)"""
import ctypes as C
import importlib.util
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sge_amd.h")
VARIANTS_HEADER = os.path.join(ROOT, "include", "sge_amd_variants.h")
VARIANT_BLAS_HEADER = os.path.join(ROOT, "include", "sge_amd_variant_blas.h")
SCENE_HEADER = os.path.join(ROOT, "include", "sge_amd_ray_scene.h")

TEN = ["sge_scene_mesh_upload", "sge_scene_mesh_info_get", "sge_scene_mesh_bounds_download", "sge_scene_instances_set",
       "sge_scene_instances_update", "sge_scene_info_get", "sge_scene_intersect_batch", "sge_scene_intersect_device",
       "sge_scene_occluded_batch", "sge_scene_occluded_device"]


@pytest.fixture(scope="module")
def lib(sge):
    import __graft_entry__
    __graft_entry__.build()
    return sge.abi.load_library()


@pytest.fixture(scope="module")
def kernels(sge, lib):
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    return kr, kr.kernel_table(sge.abi.library_path())


def declared_functions(path):
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(sge_[a-z0-9_]+)\s*\(", text)))


def test_header_mirror_and_exports_agree(sge, lib):
    names = declared_functions(SCENE_HEADER)
    assert names == sorted(TEN)
    assert names == sorted(sge.abi.SCENE_PROTOTYPES), set(names) ^ set(sge.abi.SCENE_PROTOTYPES)
    out = subprocess.check_output(["nm", "-D", "--defined-only", sge.abi.library_path()], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert set(names) <= exported
    for name in names:
        assert getattr(lib, name).argtypes == sge.abi.SCENE_PROTOTYPES[name][1], name
    text = open(SCENE_HEADER).read()
    assert re.search(r"#define SGE_HAS_RAY_SCENE 1\b", text) and '#include "sge_amd.h"' in text
    assert re.search(r"#define SGE_SCENE_STATIC_BASE 0x40000000\b", text) and sge.abi.SCENE_STATIC_BASE == 0x40000000
    assert re.search(r"#define SGE_MAX_SCENE_MESHES 64\b", text) and sge.abi.SGE_MAX_SCENE_MESHES == 64
    assert re.search(r"#define SGE_MAX_SCENE_INSTANCES 262144\b", text) and sge.abi.SGE_MAX_SCENE_INSTANCES == 262144


def test_scene_info_matches_the_header(sge, tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sge_amd_ray_scene.h"\nint main(void){'
                   'printf("%zu %zu %zu %zu %zu\\n", sizeof(struct sge_scene_info), offsetof(struct sge_scene_info, meshes), '
                   'offsetof(struct sge_scene_info, staticInstances), offsetof(struct sge_scene_info, characters), '
                   'offsetof(struct sge_scene_info, crowdReady));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    S = sge.abi.SceneInfo
    assert got == [C.sizeof(S), S.meshes.offset, S.staticInstances.offset, S.characters.offset, S.crowdReady.offset] and got[0] == 16


def test_the_older_headers_are_untouched(sge, lib):
    assert declared_functions(HEADER) == sorted(sge.abi.PROTOTYPES)
    assert declared_functions(VARIANTS_HEADER) == sorted(sge.abi.VARIANT_PROTOTYPES) and len(sge.abi.VARIANT_PROTOTYPES) == 7
    assert declared_functions(VARIANT_BLAS_HEADER) == sorted(sge.abi.VARIANT_BLAS_PROTOTYPES) and len(sge.abi.VARIANT_BLAS_PROTOTYPES) == 6
    new = set(sge.abi.SCENE_PROTOTYPES)
    for older in (sge.abi.PROTOTYPES, sge.abi.VARIANT_PROTOTYPES, sge.abi.VARIANT_BLAS_PROTOTYPES):
        assert not new & set(older)
    for path in (HEADER, VARIANTS_HEADER, VARIANT_BLAS_HEADER):
        assert not new & set(declared_functions(path)) and "sge_scene" not in open(path).read()
    assert lib.sge_abi_version() == 2 and re.search(r"#define SGE_ABI_VERSION 2\b", open(HEADER).read())


def test_new_kernels_spill_nothing_and_fit_beside_the_resident_waves(kernels):
    """scene_trace_kernel x 2 layouts, scene_occlusion_kernel x 2, scene_instance_boxes_kernel x 1: no scratch, no spills, no
    dynamic stack and at most 128 registers, the bar move_kernel<0> is held to, so that a wave of rays fits beside resident LBS
    waves. (The uniform blas_intersect_kernel needs 75 / 87.) None of the names matches a fragment an older test counts."""
    _, tab = kernels
    new = {}
    for frag, count in (("scene_trace_kernel", 2), ("scene_occlusion_kernel", 2), ("scene_instance_boxes_kernel", 1)):
        hits = {k: v for k, v in tab.items() if frag in k}
        assert len(hits) == count, (frag, sorted(hits))
        new.update(hits)
    for name, r in new.items():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and not r["dynamic_stack"], (name, r)
        assert r["vgpr"] <= 128, (name, r)
        for other in ("skin_kernel", "pose_kernel", "move_kernel", "move_group_kernel", "skin_ticket", "blas_refit_kernel", "blas_intersect_kernel",
                      "blas_world_boxes_kernel", "blas_refit_ragged_kernel", "blas_intersect_ragged_kernel", "blas_world_boxes_ragged_kernel",
                      "skin_variant_kernel", "variant_plan_kernel", "lod_select_kernel"):
            assert other not in name
    # the kernels the refactor touched are still there, once per instance
    assert len([k for k in tab if "blas_intersect_kernel" in k]) == 2 and len([k for k in tab if "blas_world_boxes_kernel" in k]) == 1
