"""CPU tests of the texture additions to the C ABI (include/sge_amd_render_textures.h): the new header, its ctypes mirror and the
library agree; the struct is 32 bytes; the older headers and their exports are what they were; the textured kernels use no scratch
and the untextured ones keep their figures. (A context needs a GPU: the argument contract is in test_gpu_render_textures.py.)"""
import ctypes as C
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "sge_amd_render_textures.h")
OLDER = {"sge_amd.h": "PROTOTYPES", "sge_amd_variants.h": "VARIANT_PROTOTYPES", "sge_amd_variant_blas.h": "VARIANT_BLAS_PROTOTYPES",
         "sge_amd_ray_scene.h": "SCENE_PROTOTYPES", "sge_amd_render.h": "RENDER_PROTOTYPES", "sge_amd_variant_scene.h": "VARIANT_SCENE_PROTOTYPES"}
COUNTS = {"sge_amd_variants.h": 7, "sge_amd_variant_blas.h": 6, "sge_amd_ray_scene.h": 10, "sge_amd_render.h": 6, "sge_amd_variant_scene.h": 1}
SEVEN = ["sge_render_material_textures_set", "sge_render_srgb_table_get", "sge_render_texture_clear", "sge_render_texture_info_get",
         "sge_render_texture_sample_batch", "sge_render_texture_sample_device", "sge_render_texture_upload"]


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
    assert names == SEVEN == sorted(sge.abi.RENDER_TEXTURE_PROTOTYPES)
    out = subprocess.check_output(["nm", "-D", "--defined-only", sge.abi.library_path()], text=True)
    assert set(names) <= {l.split()[-1] for l in out.splitlines() if " T " in l}
    for name in names:
        assert getattr(lib, name).argtypes == sge.abi.RENDER_TEXTURE_PROTOTYPES[name][1], name
    text = open(HEADER).read()
    assert re.search(r"#define SGE_HAS_RENDER_TEXTURES 1\b", text) and '#include "sge_amd_render.h"' in text
    for word, value, mirror in (("SGE_MAX_RENDER_TEXTURES", 32, sge.abi.SGE_MAX_RENDER_TEXTURES), ("SGE_TEX_RGBA8_UNORM", 0, sge.abi.TEX_RGBA8_UNORM),
                                ("SGE_TEX_RGBA8_UNORM_SRGB", 1, sge.abi.TEX_RGBA8_UNORM_SRGB), ("SGE_MAX_TEXTURE_DIM", 8192, sge.abi.SGE_MAX_TEXTURE_DIM)):
        assert re.search(r"#define %s %d\b" % (word, value), text) and mirror == value, word
    for word in ("clamp-to-edge", "fmaxf", "0.04045", "top * (1 - fy) + bot * fy", "4 + max(normalScale - 4, 0) * 0.25"):
        assert word in text, word
    for method in ("render_texture_upload", "render_texture_clear", "render_texture_info", "render_material_textures", "render_srgb_table",
                   "render_texture_sample", "render_texture_sample_device"):
        assert hasattr(sge.CharacterEngine, method), method
    d = sge.abi.default_render_material_textures(2)[1]
    assert [int(d[f]) for f in ("baseColor", "normal", "metallicRoughness", "emissive", "occlusion")] == [-1] * 5 and d["normalScale"] == 1


def test_the_struct_matches_the_header(sge, tmp_path):
    st, dt = sge.abi.RenderMaterialTextures, sge.abi.render_material_textures_dtype
    lines = ['printf("%zu", sizeof(struct sge_render_material_textures));']
    for field, _t in st._fields_:
        lines.append('printf(" %%zu", offsetof(struct sge_render_material_textures, %s));' % field)
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sge_amd_render_textures.h"\nint main(void){%s return 0;}\n' % "".join(lines))
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-I", INCLUDE, str(src), "-o", str(exe)])
    row = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert [f for f, _ in st._fields_] == ["baseColor", "normal", "metallicRoughness", "emissive", "occlusion", "normalScale", "pad"]
    assert row[0] == 32 == C.sizeof(st) == dt.itemsize
    assert row[1:] == [getattr(st, f).offset for f, _ in st._fields_] == [dt.fields[f][1] for f, _ in st._fields_] == [0, 4, 8, 12, 16, 20, 24]


# sha256 (first 16 digits) of each older header with its comments removed and its white space collapsed: everything they declare
# and define, as it stood before this header was added (the one permitted change is inside sge_amd_render.h's opening comment)
DECLARED = {'sge_amd.h': '6bdd28f6f5d95269', 'sge_amd_variants.h': '3d220440a66f5725', 'sge_amd_variant_blas.h': 'd2f51f0e26b7dc2c', 'sge_amd_ray_scene.h': 'cd48362afc52e8b4', 'sge_amd_render.h': 'f0fb525aa533dcce', 'sge_amd_variant_scene.h': '9db8670e156803f4'}


def test_the_older_headers_declare_what_they_declared():
    import hashlib
    for header, digest in DECLARED.items():
        text = re.sub(r"/\*.*?\*/", "", open(os.path.join(INCLUDE, header)).read(), flags=re.S)
        assert hashlib.sha256(" ".join(text.split()).encode()).hexdigest()[:16] == digest, header


def test_the_older_headers_keep_their_prototypes(sge, lib):
    new = set(sge.abi.RENDER_TEXTURE_PROTOTYPES)
    for header, table in OLDER.items():
        path = os.path.join(INCLUDE, header)
        protos = getattr(sge.abi, table)
        assert declared_functions(path) == sorted(protos), header
        assert len(protos) == COUNTS.get(header, len(protos)) and not new & set(protos)
        assert "sge_render_texture" not in re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S), header
    text = open(os.path.join(INCLUDE, "sge_amd_render.h")).read()
    assert "sge_amd_render_textures.h" in text and "No specular IBL" in text
    assert lib.sge_abi_version() == 2 and re.search(r"#define SGE_ABI_VERSION 2\b", open(os.path.join(INCLUDE, "sge_amd.h")).read())


def test_kernel_resources(sge, lib):
    """The textured instantiations (two strides each, uniform and ragged) and the sampler kernel use no scratch and spill nothing;
    the untextured frame kernels are at their figures: 127 VGPRs, 1212 bytes of LDS, no scratch."""
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    tab = kr.kernel_table(sge.abi.library_path())
    for frag, count in (("render_textured_kernel", 2), ("render_ragged_textured_kernel", 2), ("texture_sample_kernel", 1)):
        hits = {k: v for k, v in tab.items() if frag in k}
        assert len(hits) == count, (frag, sorted(hits))
        for name, r in hits.items():
            print(name, r)
            assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and not r["dynamic_stack"], (name, r)
            assert "render_frame_kernel" not in name and "render_ragged_frame_kernel" not in name
    for frag in ("render_frame_kernel", "render_ragged_frame_kernel"):
        hits = {k: v for k, v in tab.items() if frag in k}
        assert len(hits) == 2, (frag, sorted(hits))
        for name, r in hits.items():
            assert r["vgpr"] == 127 and r["lds"] == 1212 and r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, (name, r)


def test_a_null_context_is_refused_before_any_device_call(sge, lib):
    p = sge.abi.ptr
    buf = np.zeros(1024, np.float32)
    tex = np.zeros((2, 2, 4), np.uint8)
    w = C.c_int32(7)
    assert lib.sge_render_texture_upload(None, 0, 2, 2, 0, p(tex)) == sge.abi.SGE_ERR_INVALID
    assert lib.sge_render_texture_clear(None, -1) == sge.abi.SGE_ERR_INVALID
    assert lib.sge_render_material_textures_set(None, 1, p(sge.abi.default_render_material_textures(1))) == sge.abi.SGE_ERR_INVALID
    assert lib.sge_render_texture_info_get(None, 0, C.byref(w), C.byref(w), C.byref(w)) == sge.abi.SGE_ERR_INVALID and w.value == 7
    assert lib.sge_render_srgb_table_get(None, p(buf)) == sge.abi.SGE_ERR_INVALID and (buf == 0).all()
    assert lib.sge_render_texture_sample_batch(None, 0, p(buf), 1, p(buf)) == sge.abi.SGE_ERR_INVALID
    assert lib.sge_render_texture_sample_device(None, 0, p(buf), 1, p(buf)) == sge.abi.SGE_ERR_INVALID
    assert b"bad argument" in lib.sge_last_error()
