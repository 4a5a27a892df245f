"""CPU tests of the specular IBL additions to the C ABI (include/sge_amd_render_ibl.h): the new header, its ctypes mirror and the
library agree; the header compiles as C99; the older headers and their exports are what they were; the new kernels use no scratch
and the older frame kernels keep their figures. (A context needs a GPU: the argument contract is in test_gpu_render_ibl.py.)"""
import ctypes as C
import hashlib
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "sge_amd_render_ibl.h")
OLDER = {"sge_amd.h": "PROTOTYPES", "sge_amd_variants.h": "VARIANT_PROTOTYPES", "sge_amd_variant_blas.h": "VARIANT_BLAS_PROTOTYPES",
         "sge_amd_ray_scene.h": "SCENE_PROTOTYPES", "sge_amd_render.h": "RENDER_PROTOTYPES", "sge_amd_variant_scene.h": "VARIANT_SCENE_PROTOTYPES",
         "sge_amd_render_textures.h": "RENDER_TEXTURE_PROTOTYPES"}
COUNTS = {"sge_amd_variants.h": 7, "sge_amd_variant_blas.h": 6, "sge_amd_ray_scene.h": 10, "sge_amd_render.h": 6, "sge_amd_variant_scene.h": 1,
          "sge_amd_render_textures.h": 7}
TEN = ["sge_ibl_default_brdf_lut_build", "sge_ibl_default_env_build", "sge_render_brdf_lut_sample_batch", "sge_render_brdf_lut_sample_device",
       "sge_render_brdf_lut_upload", "sge_render_env_sample_batch", "sge_render_env_sample_device", "sge_render_env_upload",
       "sge_render_ibl_clear", "sge_render_ibl_info_get"]
# sha256 (first 16 digits) of each older header with its comments removed and its white space collapsed: everything they declare
# and define, as it stood before this header was added (the one permitted change is inside sge_amd_render.h's opening comment)
DECLARED = {'sge_amd.h': '6bdd28f6f5d95269', 'sge_amd_variants.h': '3d220440a66f5725', 'sge_amd_variant_blas.h': 'd2f51f0e26b7dc2c',
            'sge_amd_ray_scene.h': 'cd48362afc52e8b4', 'sge_amd_render.h': 'f0fb525aa533dcce', 'sge_amd_variant_scene.h': '9db8670e156803f4',
            'sge_amd_render_textures.h': 'ef857580323e0fc7'}


@pytest.fixture(scope="module")
def lib(sge):
    import __graft_entry__
    __graft_entry__.build()
    return sge.abi.load_library()


def _code(path):
    return re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)


def declared_functions(path):
    return sorted(set(re.findall(r"\b(sge_[a-z0-9_]+)\s*\(", _code(path))))


def test_header_mirror_and_exports_agree(sge, lib):
    names = declared_functions(HEADER)
    assert names == TEN == sorted(sge.abi.RENDER_IBL_PROTOTYPES)
    out = subprocess.check_output(["nm", "-D", "--defined-only", sge.abi.library_path()], text=True)
    assert set(names) <= {l.split()[-1] for l in out.splitlines() if " T " in l}
    for name in names:
        assert getattr(lib, name).argtypes == sge.abi.RENDER_IBL_PROTOTYPES[name][1], name
    text = open(HEADER).read()
    assert re.search(r"#define SGE_HAS_RENDER_IBL 1\b", text) and '#include "sge_amd_render_textures.h"' in text
    for word, value, mirror in (("SGE_MAX_ENV_SIZE", 2048, sge.abi.SGE_MAX_ENV_SIZE), ("SGE_MAX_ENV_MIPS", 12, sge.abi.SGE_MAX_ENV_MIPS),
                                ("SGE_MAX_BRDF_LUT_DIM", 4096, sge.abi.SGE_MAX_BRDF_LUT_DIM)):
        assert re.search(r"#define %s %d\b" % (word, value), text) and mirror == value, word
    for word in ("IBLResources.swift", "RayTracing.metalinc:88-104", "ax >= ay && ax >= az", "fl = mip - (float)l0", "round to nearest even",
                 "-Z (-x, -y) / az", "((direct + ambient) + spec * occlusion) + emissive", "the zero vector is face +X"):
        assert word in text, word
    for method in ("render_env_upload", "render_brdf_lut_upload", "render_ibl_clear", "render_ibl_info", "render_env_sample", "render_brdf_lut_sample",
                   "render_env_sample_device", "render_brdf_lut_sample_device"):
        assert hasattr(sge.CharacterEngine, method), method
    assert callable(sge.ibl_default_env) and callable(sge.ibl_default_brdf_lut)
    assert sge.abi.env_texel_count(8, 4) == 6 * (64 + 16 + 4 + 1) and sge.abi.env_texel_count(1, 1) == 6


def test_the_header_compiles_as_c99_without_any_struct_of_its_own(tmp_path):
    assert "struct" not in _code(HEADER).replace("struct sge_context", "")
    src = tmp_path / "h.c"
    src.write_text('#include "sge_amd_render_ibl.h"\n#if !SGE_HAS_RENDER_IBL || !SGE_HAS_RENDER_TEXTURES\n#error\n#endif\n'
                   'int (*build)(int32_t, int32_t, uint16_t*) = sge_ibl_default_env_build;\nint main(void){ return build == 0; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-c", "-I", INCLUDE, str(src), "-o", str(tmp_path / "h.o")])


def test_the_older_headers_declare_what_they_declared(sge, lib):
    for header, digest in DECLARED.items():
        assert hashlib.sha256(" ".join(_code(os.path.join(INCLUDE, header)).split()).encode()).hexdigest()[:16] == digest, header
    new = set(sge.abi.RENDER_IBL_PROTOTYPES)
    for header, table in OLDER.items():
        path = os.path.join(INCLUDE, header)
        protos = getattr(sge.abi, table)
        assert declared_functions(path) == sorted(protos), header
        assert len(protos) == COUNTS.get(header, len(protos)) and not new & set(protos)
        assert not re.search(r"sge_render_(env|brdf|ibl)|sge_ibl_", _code(path)), header
    text = open(os.path.join(INCLUDE, "sge_amd_render.h")).read()
    for word in ("No textures", "No specular IBL", "face-forwarded", "sge_amd_render_textures.h", "sge_amd_render_ibl.h"):
        assert word in text, word
    assert lib.sge_abi_version() == 2 and re.search(r"#define SGE_ABI_VERSION 2\b", open(os.path.join(INCLUDE, "sge_amd.h")).read())


def test_kernel_resources(sge, lib):
    """The IBL instantiations (two strides each: uniform and ragged, untextured and textured) and the sampler kernel use no scratch,
    spill nothing and have no dynamic stack; the four older frame-kernel families are at their counts and figures."""
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    tab = kr.kernel_table(sge.abi.library_path())
    older = ("render_frame_kernel", "render_ragged_frame_kernel", "render_textured_kernel", "render_ragged_textured_kernel", "texture_sample_kernel")
    for frag, count in (("render_ibl_kernel", 2), ("render_ibl_tex_kernel", 2), ("render_ragged_ibl_kernel", 2), ("render_ragged_ibl_tex_kernel", 2),
                        ("ibl_sample_kernel", 1)):
        hits = {k: v for k, v in tab.items() if frag in k}
        assert len(hits) == count, (frag, sorted(hits))
        for name, r in hits.items():
            print(name, r)
            assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and not r["dynamic_stack"], (name, r)
            assert not any(o in name for o in older), name
    for frag in ("render_frame_kernel", "render_ragged_frame_kernel"):
        hits = {k: v for k, v in tab.items() if frag in k}
        assert len(hits) == 2, (frag, sorted(hits))
        for name, r in hits.items():
            assert r["vgpr"] == 127 and r["lds"] == 1212 and r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, (name, r)
    for frag in ("render_textured_kernel", "render_ragged_textured_kernel"):
        hits = {k: v for k, v in tab.items() if frag in k}
        assert len(hits) == 2, (frag, sorted(hits))
        for name, r in hits.items():
            assert r["vgpr"] in (143, 144) and r["lds"] == 1300 and r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, (name, r)
    assert len([k for k in tab if "texture_sample_kernel" in k]) == 1


def test_a_null_context_is_refused_and_the_builders_check_their_arguments(sge, lib):
    p = sge.abi.ptr
    buf = np.zeros(1024, np.float32)
    w = C.c_int32(7)
    bad = sge.abi.SGE_ERR_INVALID
    assert lib.sge_render_env_upload(None, 1, 1, p(buf)) == bad
    assert lib.sge_render_brdf_lut_upload(None, 1, 1, p(buf)) == bad
    assert lib.sge_render_ibl_clear(None) == bad
    assert lib.sge_render_ibl_info_get(None, C.byref(w), C.byref(w), C.byref(w), C.byref(w)) == bad and w.value == 7
    assert lib.sge_render_env_sample_batch(None, p(buf), p(buf), 1, p(buf)) == bad
    assert lib.sge_render_brdf_lut_sample_batch(None, p(buf), 1, p(buf)) == bad
    assert lib.sge_render_env_sample_device(None, p(buf), p(buf), 1, p(buf)) == bad
    assert lib.sge_render_brdf_lut_sample_device(None, p(buf), 1, p(buf)) == bad
    assert b"bad argument" in lib.sge_last_error() and (buf == 0).all()
    for size, mips in ((0, 1), (3, 1), (4096, 1), (8, 0), (8, 5)):
        assert lib.sge_ibl_default_env_build(size, mips, p(buf)) == bad and (buf == 0).all(), (size, mips)
    assert lib.sge_ibl_default_env_build(8, 4, None) == bad
    for size, count in ((0, 16), (4097, 16), (4, 0), (4, 65537)):
        assert lib.sge_ibl_default_brdf_lut_build(size, count, p(buf)) == bad and (buf == 0).all(), (size, count)
    assert lib.sge_ibl_default_brdf_lut_build(4, 16, None) == bad
