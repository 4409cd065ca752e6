"""CPU test of the owner that holds every event, stream and buffer of a context (csrc/rt_owned.h): tests/native/
owned_check.cpp, a stand-alone program, under AddressSanitizer + UBSan.  No GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "owned_check.cpp")
HEADER = os.path.join(ROOT, "raytracing_engine_amd", "csrc", "rt_owned.h")


def test_owner_under_sanitizers(tmp_path):
    exe = tmp_path / "owned_check"
    subprocess.run(["g++", "-g", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", SRC, "-o", str(exe)],
                   check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("OK"), out.stdout + out.stderr


def test_the_owner_header_is_free_of_hip():
    """It is tested on the CPU because it includes no HIP header (the HIP instantiations are in csrc/rt_internal.h)."""
    with open(HEADER) as f:
        includes = [line for line in f if line.lstrip().startswith("#include")]
    assert not [line for line in includes if "hip" in line.lower() or "rt_internal" in line], includes
