"""CPU tests of the shaded frame's additions to the C ABI (include/sge_amd_render.h): the new header, its ctypes mirror and the
library agree; the older headers and their mirrors are what they were; render_frame_kernel uses no scratch, spills nothing and
stays inside 128 registers. (A context cannot be created without a GPU, so the argument contract is tested in test_gpu_render.py.)"""
import ctypes as C
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
RENDER_HEADER = os.path.join(INCLUDE, "sge_amd_render.h")
OLDER = {"sge_amd.h": "PROTOTYPES", "sge_amd_variants.h": "VARIANT_PROTOTYPES", "sge_amd_variant_blas.h": "VARIANT_BLAS_PROTOTYPES",
         "sge_amd_ray_scene.h": "SCENE_PROTOTYPES"}
SIX = ["sge_render_materials_set", "sge_render_static_materials", "sge_render_crowd_materials", "sge_render_lights_set",
       "sge_render_frame_batch", "sge_render_frame_device"]


@pytest.fixture(scope="module")
def lib(sge):
    import __graft_entry__
    __graft_entry__.build()
    return sge.abi.load_library()


def declared_functions(path):
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(sge_[a-z0-9_]+)\s*\(", text)))


def test_header_mirror_and_exports_agree(sge, lib):
    names = declared_functions(RENDER_HEADER)
    assert names == sorted(SIX) == sorted(sge.abi.RENDER_PROTOTYPES)
    out = subprocess.check_output(["nm", "-D", "--defined-only", sge.abi.library_path()], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert set(names) <= exported
    for name in names:
        assert getattr(lib, name).argtypes == sge.abi.RENDER_PROTOTYPES[name][1], name
    text = open(RENDER_HEADER).read()
    assert re.search(r"#define SGE_HAS_RENDER 1\b", text) and '#include "sge_amd_ray_scene.h"' in text
    assert re.search(r"#define SGE_MAX_RENDER_MATERIALS 256\b", text) and sge.abi.SGE_MAX_RENDER_MATERIALS == 256
    assert re.search(r"#define SGE_MAX_DIR_LIGHTS 8\b", text) and sge.abi.SGE_MAX_DIR_LIGHTS == 8
    assert re.search(r"#define SGE_MAX_RENDER_PIXELS 67108864\b", text) and sge.abi.SGE_MAX_RENDER_PIXELS == 1 << 26
    for word in ("No textures", "No specular IBL", "face-forwarded"):
        assert word in text
    d = sge.abi.default_render_materials(1)[0]
    assert (d["baseColor"].tolist(), d["metallic"], d["roughness"], d["emissive"].tolist(), d["occlusionStrength"], d["alpha"], d["transmission"],
            d["ior"]) == ([1, 1, 1], 0, 0.5, [0, 0, 0], 1, 1, 0, 1.5)


def test_structs_match_the_header(sge, tmp_path):
    structs = {"sge_render_material": (sge.abi.RenderMaterial, sge.abi.render_material_dtype, 48),
               "sge_render_light": (sge.abi.RenderLight, sge.abi.render_light_dtype, 48),
               "sge_render_frame": (sge.abi.RenderFrame, sge.abi.render_frame_dtype, 204),
               "sge_render_aov": (sge.abi.RenderAov, sge.abi.render_aov_dtype, 32)}
    lines = []
    for name, (st, _, _) in structs.items():
        lines.append('printf("%%zu", sizeof(struct %s));' % name)
        for field, _t in st._fields_:
            lines.append('printf(" %%zu", offsetof(struct %s, %s));' % (name, field))
        lines.append('printf("\\n");')
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sge_amd_render.h"\nint main(void){%s return 0;}\n' % "".join(lines))
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-I", INCLUDE, str(src), "-o", str(exe)])
    rows = [[int(x) for x in l.split()] for l in subprocess.check_output([str(exe)], text=True).splitlines()]
    for row, (name, (st, dt, size)) in zip(rows, structs.items()):
        assert row[0] == size == C.sizeof(st) == dt.itemsize, name
        assert row[1:] == [getattr(st, f).offset for f, _ in st._fields_] == [dt.fields[f][1] for f, _ in st._fields_], name


def test_the_older_headers_are_untouched(sge, lib):
    new = set(sge.abi.RENDER_PROTOTYPES)
    counts = {"sge_amd_variants.h": 7, "sge_amd_variant_blas.h": 6, "sge_amd_ray_scene.h": 10}
    for header, table in OLDER.items():
        path = os.path.join(INCLUDE, header)
        protos = getattr(sge.abi, table)
        assert declared_functions(path) == sorted(protos), header
        assert header not in counts or len(protos) == counts[header]
        assert not new & set(protos) and "sge_render" not in open(path).read()
    assert lib.sge_abi_version() == 2 and re.search(r"#define SGE_ABI_VERSION 2\b", open(os.path.join(INCLUDE, "sge_amd.h")).read())


def test_the_render_kernel_spills_nothing_and_stays_inside_128_registers(sge, lib):
    """render_frame_kernel x 2 crowd strides: no scratch, no VGPR or SGPR spills, no dynamic stack, at most 128 VGPRs (the bar of the
    ray kernels). The scene kernels it shares device code with are still there, once per instance."""
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    tab = kr.kernel_table(sge.abi.library_path())
    hits = {k: v for k, v in tab.items() if "render_frame_kernel" in k}
    assert len(hits) == 2, sorted(hits)
    for name, r in hits.items():
        print(name, r)
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and not r["dynamic_stack"], (name, r)
        assert r["vgpr"] <= 128, (name, r)
    for frag, count in (("scene_trace_kernel", 2), ("scene_occlusion_kernel", 2), ("scene_instance_boxes_kernel", 1)):
        assert len([k for k in tab if frag in k]) == count, frag


def test_a_null_context_is_refused_before_any_device_call(sge, lib):
    """The argument contract that needs no device: every entry point returns SGE_ERR_INVALID for a NULL context (the rest of the
    contract needs a context, which needs a GPU: test_gpu_render.py)."""
    f = sge.CharacterEngine.render_frame_record(np.eye(4), (0, 0, 0), 4, 4, 0)
    buf = np.zeros(64, np.float32)
    p = sge.abi.ptr
    assert lib.sge_render_materials_set(None, 1, p(sge.abi.default_render_materials(1))) == sge.abi.SGE_ERR_INVALID
    assert lib.sge_render_static_materials(None, 0, None) == sge.abi.SGE_ERR_INVALID
    assert lib.sge_render_crowd_materials(None, 0, None) == sge.abi.SGE_ERR_INVALID
    assert lib.sge_render_lights_set(None, 0, None) == sge.abi.SGE_ERR_INVALID
    assert lib.sge_render_frame_batch(None, p(f), p(buf), None) == sge.abi.SGE_ERR_INVALID and (buf == 0).all()
    assert lib.sge_render_frame_device(None, p(f), p(buf), None) == sge.abi.SGE_ERR_INVALID
    assert b"bad argument" in lib.sge_last_error()
