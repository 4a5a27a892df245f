"""sge::RayTracingRenderer of the C++ host mirror (swift-game-engine_amd/host/sge_host.hpp): it compiles against the public headers and
links against the product library (CPU check), and renders on a GPU (tests/cpp/render_mirror_smoke.cpp)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "swift-game-engine_amd")
SRC = os.path.join(ROOT, "tests", "cpp", "render_mirror_smoke.cpp")


def build(tmp_path):
    import __graft_entry__
    __graft_entry__.build()
    exe = str(tmp_path / "render_mirror_smoke")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", SRC, "-I" + os.path.join(ROOT, "include"), "-L" + PKG, "-lsge_amd",
                           "-Wl,-rpath," + PKG, "-o", exe])
    return exe


def test_render_mirror_compiles_links_and_inverts(tmp_path, sge):
    """Without a device the program checks inverse4 and stops with status 2 before the GPU part."""
    out = subprocess.run([build(tmp_path)], capture_output=True, text=True, timeout=120)
    assert out.returncode in (0, 2), out.stdout + out.stderr
    assert "FAILED" not in out.stdout


@pytest.mark.gpu
def test_render_mirror_on_gpu(tmp_path, sge):
    out = subprocess.run([build(tmp_path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "render mirror smoke ok" in out.stdout
