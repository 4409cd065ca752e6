"""CPU tests of the two headers the host BVH builders share: the node format with its quantiser and slot assignment
(csrc/bvh_node.h, tests/native/bvh_node_check.cpp, AddressSanitizer + UBSan) and the thread helper (csrc/host_parallel.h,
tests/native/parallel_for_check.cpp, AddressSanitizer + UBSan and ThreadSanitizer).  No GPU."""
import os
import subprocess

import pytest

from test_bvh_build_host import run_tsan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ASAN_UBSAN = ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
TSAN = ["-O2", "-fsanitize=thread"]


def build_and_run(tmp_path, name, flags):
    exe = tmp_path / name
    src = os.path.join(ROOT, "tests", "native", name + ".cpp")
    subprocess.run(["g++", "-g", "-std=c++17", "-pthread", "-Wall", "-Wextra", "-Werror"] + flags + [src, "-o", str(exe)], check=True)
    return run_tsan([str(exe)])


def test_quantise_and_assign_slots_under_sanitizers(tmp_path):
    out = build_and_run(tmp_path, "bvh_node_check", ASAN_UBSAN)
    assert out.returncode == 0 and out.stdout.startswith("OK"), out.stdout + out.stderr


@pytest.mark.parametrize("flags", [ASAN_UBSAN, TSAN], ids=["asan_ubsan", "tsan"])
def test_parallel_for_carries_exceptions_back_after_the_join(tmp_path, flags):
    out = build_and_run(tmp_path, "parallel_for_check", flags)
    assert out.returncode == 0 and out.stdout.startswith("OK") and "ThreadSanitizer" not in out.stderr, out.stdout + out.stderr
