"""CPU tests of the per-variant acceleration structures' additions to the C ABI (include/sge_amd_variant_blas.h): the new header,
its ctypes mirror and the library agree; the older headers, abi.PROTOTYPES, abi.VARIANT_PROTOTYPES and the oracle binding are what
they were; the new kernels use no scratch and keep the occupancy of the uniform refit."""
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
VARIANT_BLAS_HEADER = os.path.join(ROOT, "include", "sge_amd_variant_blas.h")


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
    names = declared_functions(VARIANT_BLAS_HEADER)
    assert len(names) == 6
    assert names == sorted(sge.abi.VARIANT_BLAS_PROTOTYPES), set(names) ^ set(sge.abi.VARIANT_BLAS_PROTOTYPES)
    out = subprocess.check_output(["nm", "-D", "--defined-only", sge.abi.library_path()], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert set(names) <= exported
    for name in names:
        assert getattr(lib, name).argtypes == sge.abi.VARIANT_BLAS_PROTOTYPES[name][1], name
    text = open(VARIANT_BLAS_HEADER).read()
    assert re.search(r"#define SGE_HAS_VARIANT_BLAS 1\b", text) and '#include "sge_amd_variants.h"' in text


def test_layout_struct_matches_the_header(sge, tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sge_amd_variant_blas.h"\nint main(void){'
                   'printf("%zu %zu %zu %zu %zu\\n", sizeof(struct sge_blas_variant_layout), offsetof(struct sge_blas_variant_layout, ready), '
                   'offsetof(struct sge_blas_variant_layout, variants), offsetof(struct sge_blas_variant_layout, rowStride), '
                   'offsetof(struct sge_blas_variant_layout, entryCount));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    L = sge.abi.BlasVariantLayout
    assert got == [C.sizeof(L), L.ready.offset, L.variants.offset, L.rowStride.offset, L.entryCount.offset] and got[0] == 48
    assert L.entryCount.size == 4 * sge.abi.SGE_MAX_MESH_VARIANTS


def test_the_older_headers_are_untouched(sge, lib):
    assert declared_functions(HEADER) == sorted(sge.abi.PROTOTYPES)
    assert declared_functions(VARIANTS_HEADER) == sorted(sge.abi.VARIANT_PROTOTYPES) and len(sge.abi.VARIANT_PROTOTYPES) == 7
    new = set(sge.abi.VARIANT_BLAS_PROTOTYPES)
    assert not new & set(sge.abi.PROTOTYPES) and not new & set(sge.abi.VARIANT_PROTOTYPES)
    assert not new & set(declared_functions(HEADER)) and not new & set(declared_functions(VARIANTS_HEADER))
    assert lib.sge_abi_version() == 2 and re.search(r"#define SGE_ABI_VERSION 2\b", open(HEADER).read())
    assert ob.load_oracle() is not None


def test_new_kernels_use_no_scratch_and_keep_the_refit_s_occupancy(kernels):
    """No scratch, no spills, no dynamic stack for every new kernel. The ragged refit leaves as many wavefronts per SIMD as
    blas_refit_kernel of the same template arguments in the same library, or the six that three 512-thread workgroups per CU
    need, whichever is smaller."""
    kr, tab = kernels
    ragged = {k: v for k, v in tab.items() if "blas_refit_ragged_kernel" in k}
    assert len(ragged) == 6, sorted(ragged)                  # two layouts x three tile capacities
    for name, r in ragged.items():
        twin = name.replace("blas_refit_ragged_kernel", "blas_refit_kernel")
        args = re.search(r"ILi(\d)ELi(\d+)E", name).groups()
        uniform = [v for k, v in tab.items() if "blas_refit_kernel" in k and "ILi%sELi%sE" % args in k]
        assert len(uniform) == 1, (name, twin)
        need = min(kr.waves_per_simd(uniform[0]["vgpr"]), 6)
        assert kr.waves_per_simd(r["vgpr"]) >= need, (name, r["vgpr"], uniform[0]["vgpr"])
    new = dict(ragged)
    for frag, count in (("blas_intersect_ragged_kernel", 2), ("blas_world_boxes_ragged_kernel", 1)):
        hits = {k: v for k, v in tab.items() if frag in k}
        assert len(hits) == count, (frag, sorted(hits))
        new.update(hits)
    for name, r in new.items():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and not r["dynamic_stack"], (name, r)
        for other in ("skin_variant_kernel", "variant_plan_kernel", "lod_select_kernel"):
            assert other not in name


def test_the_variant_skin_kernels_are_still_six(kernels):
    _, tab = kernels
    assert len([k for k in tab if "skin_variant_kernel" in k]) == 6
    assert len([k for k in tab if "variant_plan_kernel" in k]) == 1 and len([k for k in tab if "lod_select_kernel" in k]) == 1
    # the uniform refit / closest-hit / world-box kernels are all still there, once per instance
    assert len([k for k in tab if "blas_refit_kernel" in k]) == 6 and len([k for k in tab if "blas_intersect_kernel" in k]) == 2
    assert len([k for k in tab if "blas_world_boxes_kernel" in k]) == 1
