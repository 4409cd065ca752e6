"""What every native reference of the tests shares: building tests/native/<name>.cpp, running the program on raw array files, and
cutting its output file into typed arrays.

Test helper (imported by the *_exact.py modules and tests/transport_ref.py the way they import each other); not a conftest, no
fixtures.  What a reference computes, its cases and its contract stay in its own module: here is only the plumbing they had a copy
of each."""
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
BVH_BUILD = os.path.join(ROOT, "raytracing_engine_amd", "csrc", "bvh_build.cpp")  # for the programs that walk the host-built tree
PLAIN = ("-O2",)
SANITIZED = ("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
OUT = object()  # run(): the value that marks where the output file's path goes, for a program that does not take it last

_BUILT = {}


def build(name, sources=(), sanitized=False, where=None, flags=()):
    """Compiles tests/native/<name>.cpp and `sources` with g++ -std=c++17 -ffp-contract=off, `flags` (-pthread, warnings) and -O2,
    or, sanitized, with ASan + UBSan into a stand-alone program <name>_asan; once per process and flavour, in `where` (default: a new
    temporary directory).  Returns the program's path."""
    if (name, sanitized) not in _BUILT:
        where = where or tempfile.mkdtemp(prefix=name + "_")
        exe = os.path.join(where, name + "_asan" if sanitized else name)
        subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", *flags, *(SANITIZED if sanitized else PLAIN),
                        os.path.join(NATIVE, name + ".cpp"), *sources, "-o", exe], check=True)
        _BUILT[name, sanitized] = exe
    return _BUILT[name, sanitized]


def run(exe, inputs):
    """Runs `exe <inputs...> out` in a fresh temporary directory and returns the bytes of out.  `inputs` maps, in the order of the
    command line, a file name to an array (written raw under that name), to None (the program gets "-"), to a str (the program gets
    that word: a mode, a thread count) or to OUT (the output path comes here and not last).  RuntimeError unless the program
    returns 0 and its stdout starts with OK."""
    with tempfile.TemporaryDirectory(prefix=os.path.basename(exe) + "_") as d:
        out = os.path.join(d, "out")
        cmd = [exe]
        for name, a in inputs.items():
            if a is OUT:
                cmd.append(out)
            elif a is None or isinstance(a, str):
                cmd.append("-" if a is None else a)
            else:
                np.ascontiguousarray(a).tofile(os.path.join(d, name))
                cmd.append(os.path.join(d, name))
        if out not in cmd:
            cmd.append(out)
        done = subprocess.run(cmd, capture_output=True, text=True)
        if done.returncode != 0 or not done.stdout.startswith("OK"):
            raise RuntimeError(f"{os.path.basename(exe)} failed ({done.returncode}): {done.stdout}{done.stderr}")
        with open(out, "rb") as f:
            return f.read()


def unpack(raw, head_words, fields):
    """(head, arrays) of an output file: head_words uint64, then the arrays of `fields` one after the other.  `fields` is a sequence
    of (key, dtype, count), or a function of the head (a tuple of ints) that returns one, where the counts stand in the head.  Every
    array is a copy, and the whole stream must be consumed."""
    buf = np.frombuffer(raw, np.uint8)
    assert len(buf) >= 8 * head_words, (len(buf), head_words)
    head = tuple(int(x) for x in buf[:8 * head_words].view(np.uint64))
    out, at = {}, 8 * head_words
    for key, dt, count in (fields(head) if callable(fields) else fields):
        size = count * np.dtype(dt).itemsize
        assert at + size <= len(buf), (key, at, size, len(buf))
        out[key] = buf[at:at + size].view(dt).copy()
        at += size
    assert at == len(buf), (at, len(buf))
    return head, out


def same_bits(a, b, same_dtype=False):
    """Two arrays of one shape agree, float32 ones bit for bit (NaN equals the same NaN, -0.0 is not 0.0); with same_dtype, arrays
    of different integer types do not agree either."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or (a.dtype != b.dtype and (same_dtype or a.dtype == np.float32)):
        return False
    if a.dtype == np.float32:
        return bool(np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32)))
    return bool(np.array_equal(a, b))
