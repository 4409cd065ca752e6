"""The boundary of one query kind, described once (Kind) and checked once: its C functions are exported and bound, a NULL context
is refused, the ctypes mirrors of its structs lie as include/rt_abi.h lays them out, its default parameters are zeros; and the
renderer that takes CPU tensors for its device's (cpu_renderer), with which a wrapper's refusals are reached without a GPU.

Test helper (imported by the tests/test_*_host.py files of the query kinds); not a conftest, no fixtures."""
import ctypes as C
import dataclasses
import os
import subprocess

import raytracing_engine_amd as R
from raytracing_engine_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ABI_VERSION = 4  # additions only


@dataclasses.dataclass(frozen=True)
class Kind:
    """One query kind at the C boundary.  params / stats: the names of its ctypes classes in raytracing_engine_amd (None: the kind has
    no such struct); params_c / stats_c: the structs' names in rt_abi.h; params_fields / stats_fields: the members in order (a
    frozenset: in any order); constants: header macro -> the value Python holds for it; null_calls: (function, arguments behind the
    NULL context) of calls that must return RT_ERR_INVALID; default: the function that fills the default parameters."""
    functions: tuple
    methods: tuple = ()
    params: str = None
    stats: str = None
    params_c: str = None
    stats_c: str = None
    params_fields: object = None
    stats_fields: object = None
    constants: dict = dataclasses.field(default_factory=dict)
    null_calls: tuple = ()
    default: str = None

    def structs(self):
        """[(ctypes class, C name, expected members)] of the structs the kind has."""
        return [(getattr(R, cls), c_name, fields) for cls, c_name, fields in
                ((self.params, self.params_c, self.params_fields), (self.stats, self.stats_c, self.stats_fields)) if cls is not None]


# the test hook that returns path A's secondary marches (rt_render_chains; no struct of its own)
CHAIN_HOOK = Kind(functions=("rt_render_chains",), methods=("render_chains",), null_calls=(("rt_render_chains", (None, None, None, None, None)),))


def exports(kind):
    lib = R.load()
    for name in kind.functions:
        assert hasattr(lib, name), name
        assert name in _lib.PROTOTYPES, name
    assert lib.rt_abi_version() == ABI_VERSION
    for method in kind.methods:
        assert callable(getattr(R.Renderer, method)), method
    for cls in (kind.params, kind.stats):
        assert cls is None or getattr(R, cls) is getattr(_lib, cls), cls


def null_context(kind):
    lib = R.load()
    assert kind.null_calls
    for name, args in kind.null_calls:
        assert name in kind.functions, name
        assert getattr(lib, name)(None, *args) == -1, (name, args)  # RT_ERR_INVALID: nothing touched


def struct_layout(kind, tmp_path, structs=None):
    """sizeof / offsetof as gcc computes them from include/rt_abi.h, and the header's constants, against the ctypes mirrors and the
    expected member lists.  `structs`: other [(ctypes class, C name, expected members)] than the kind's own (the self-test's)."""
    structs = kind.structs() if structs is None else structs
    assert structs
    names = [[n for n, _ in cls._fields_] for cls, _, _ in structs]
    macros = ["RT_ABI_VERSION"] + list(kind.constants)
    prog = tmp_path / "layout.c"
    prog.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"rt_abi.h\"\nint main(void) {\n"
                    + "".join(f"    printf(\"%lld\\n\", (long long)({m}));\n" for m in macros)
                    + "".join(f"    printf(\"%zu\\n\", sizeof({c_name}));\n" + "".join(f"    printf(\"%zu\\n\", offsetof({c_name}, {n}));\n" for n in members)
                              for (_, c_name, _), members in zip(structs, names))
                    + "    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out[:len(macros)] == [ABI_VERSION] + list(kind.constants.values()), (macros, out[:len(macros)])
    at = len(macros)
    for (cls, c_name, expected), members in zip(structs, names):
        assert out[at:at + 1 + len(members)] == [C.sizeof(cls)] + [getattr(cls, n).offset for n in members], c_name
        at += 1 + len(members)
        assert (frozenset(members) == expected and len(members) == len(expected)) if isinstance(expected, frozenset) else members == list(expected), (c_name, members)
    assert at == len(out)


def default_params(kind):
    lib = R.load()
    cls = getattr(R, kind.params)
    p = cls(*[7] * len(cls._fields_))
    assert bytes(p) != bytes(C.sizeof(cls))
    assert getattr(lib, kind.default)(C.byref(p)) == 0
    assert bytes(p) == bytes(C.sizeof(cls))


class OnCpu(R.Renderer):
    """A renderer whose tensor checks are Renderer's own, told that every tensor lies on its device: a CPU tensor of the right type,
    layout and shape passes, so that what a wrapper refuses behind those checks is reached without a GPU (tests/test_support_host.py
    compares the two)."""

    def _on_device(self, t):
        return True


def cpu_renderer():
    """An OnCpu without a context and without a library: whatever gets past the wrapper's checks fails on None."""
    r = OnCpu.__new__(OnCpu)
    r._lib, r._ctx, r.device = None, None, 0
    return r
