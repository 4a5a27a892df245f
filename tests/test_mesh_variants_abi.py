"""CPU tests of the mesh-variant additions to the C ABI (include/sge_amd_variants.h): the new header, its ctypes mirror and the
library agree; include/sge_amd.h, abi.PROTOTYPES and the oracle binding are what they were; the new kernels keep inside the
resources the overlap schedule counts on."""
import ctypes as C
import importlib.util
import os
import re
import subprocess

import pytest

import oracle_binding as ob

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sge_amd.h")
VARIANTS_HEADER = os.path.join(ROOT, "include", "sge_amd_variants.h")


@pytest.fixture(scope="module")
def lib(sge):
    import __graft_entry__
    __graft_entry__.build()
    return sge.abi.load_library()


def declared_functions(path):
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(sge_[a-z0-9_]+)\s*\(", text)))


def test_variant_header_mirror_and_exports_agree(sge, lib):
    names = declared_functions(VARIANTS_HEADER)
    assert len(names) == 7
    assert names == sorted(sge.abi.VARIANT_PROTOTYPES), set(names) ^ set(sge.abi.VARIANT_PROTOTYPES)
    out = subprocess.check_output(["nm", "-D", "--defined-only", sge.abi.library_path()], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert set(names) <= exported
    for name in names:
        assert getattr(lib, name).argtypes == sge.abi.VARIANT_PROTOTYPES[name][1], name
    text = open(VARIANTS_HEADER).read()
    assert re.search(r"#define SGE_HAS_MESH_VARIANTS 1\b", text) and re.search(r"#define SGE_MAX_MESH_VARIANTS 8\b", text)
    assert sge.abi.SGE_MAX_MESH_VARIANTS == 8


def test_plan_info_layout_matches_the_header(sge, tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sge_amd_variants.h"\nint main(void){'
                   'printf("%zu %zu %zu %zu\\n", sizeof(sge_skin_plan_info), offsetof(sge_skin_plan_info, perVariant), '
                   'offsetof(sge_skin_plan_info, units), offsetof(sge_skin_plan_info, charsPerUnit));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    P = sge.abi.SkinPlanInfo
    assert got == [C.sizeof(P), P.perVariant.offset, P.units.offset, P.charsPerUnit.offset] and got[0] == 64


def test_the_existing_abi_is_untouched(sge, lib):
    """The additions live beside include/sge_amd.h, not in it: that header still declares exactly abi.PROTOTYPES, none of the new
    names has leaked into either, the ABI version is 2 and the oracle (which binds every entry of abi.PROTOTYPES) still loads."""
    assert declared_functions(HEADER) == sorted(sge.abi.PROTOTYPES)
    assert not set(sge.abi.VARIANT_PROTOTYPES) & set(sge.abi.PROTOTYPES)
    assert not set(sge.abi.VARIANT_PROTOTYPES) & set(declared_functions(HEADER))
    assert lib.sge_abi_version() == 2 and re.search(r"#define SGE_ABI_VERSION 2\b", open(HEADER).read())
    assert ob.load_oracle() is not None


def test_variant_kernels_keep_inside_the_schedule_s_resources(sge, lib):
    """skin_variant_kernel runs where skin_ticket_multi_kernel<3, 4> runs, beside the next step's collision kernels: <= 96 vector
    registers, no scratch, no dynamic stack, for every instance. The plan and LOD kernels: no scratch, no dynamic stack."""
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    tab = kr.kernel_table(sge.abi.library_path())
    skin = {k: v for k, v in tab.items() if "skin_variant_kernel" in k}
    assert len(skin) == 6, sorted(skin)                      # two output layouts x 1, 2 or 4 characters per unit
    for name, r in skin.items():
        assert "skin_kernel" not in name and "skin_ticket_kernel" not in name
        assert r["vgpr"] <= 96 and r["scratch"] == 0 and r["vgpr_spill"] == 0 and not r["dynamic_stack"], (name, r)
    for frag in ("variant_plan_kernel", "lod_select_kernel"):
        hits = {k: v for k, v in tab.items() if frag in k}
        assert len(hits) == 1, (frag, sorted(hits))
        for name, r in hits.items():
            assert r["scratch"] == 0 and not r["dynamic_stack"], (name, r)


def test_decimated_variant_keeps_consistent_bone_data(sge, ybot):
    import numpy as np
    B = ybot.bone_count
    bind = np.tile(np.eye(4, dtype=np.float32).reshape(16), (B, 1))
    bind[:, 12:15] = np.random.default_rng(1).normal(0, 1, (B, 3))
    mesh = sge.assets.make_synthetic_skinned_mesh(ybot.parent, bind, rings=6, segments=6)
    V = mesh["positions"].shape[0]
    for keep in (0.5, 0.25, 1, V):
        d = sge.assets.decimate_skinned_mesh(mesh, keep)
        n = d["positions"].shape[0]
        assert n == (keep if isinstance(keep, int) else round(V * keep))
        assert all(d[k].shape[0] == n for k in ("normals", "uvs", "boneIndices", "boneWeights"))
        assert d["boneIndices"].max() < B and np.allclose(d["boneWeights"].sum(1), 1.0, atol=1e-5)
        assert d["indices"].size % 3 == 0 and (d["indices"].size == 0 or d["indices"].max() < n)
        rows = (np.arange(n, dtype=np.int64) * V) // n
        assert np.array_equal(d["positions"], mesh["positions"][rows]) and np.array_equal(d["boneIndices"], mesh["boneIndices"][rows])
    assert np.array_equal(sge.assets.decimate_skinned_mesh(mesh, V)["indices"], mesh["indices"])
