"""CPU test of the mesh key and the table of resident meshes (csrc/mesh_registry.h), which decide whether two
contexts share one device mesh: tests/native/mesh_registry_check.cpp under AddressSanitizer + UBSan, and its threads under
ThreadSanitizer.  No GPU."""
import os
import subprocess

import pytest

from raytracing_engine_amd import _lib
from test_bvh_build_host import run_tsan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "mesh_registry_check.cpp")


@pytest.mark.parametrize("flags", [["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], ["-O2", "-fsanitize=thread"]], ids=["asan_ubsan", "tsan"])
def test_key_and_registry_under_sanitizers(tmp_path, flags):
    exe = tmp_path / "mesh_registry_check"
    subprocess.run(["g++", "-g", "-std=c++17", "-pthread", "-Wall", "-Wextra", "-Werror"] + flags + [SRC, "-o", str(exe)], check=True)
    out = run_tsan([str(exe)])
    assert out.returncode == 0 and out.stdout.startswith("OK"), out.stdout + out.stderr


def test_binding_has_the_query():
    assert "rt_mesh_sharers" in _lib.PROTOTYPES
