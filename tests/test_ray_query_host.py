"""CPU tests of the ray-query boundary (rt_query_rays_device / Renderer.query_rays): the library exports and binds the three
functions, a NULL context is refused without a GPU, the two structs have the layout gcc gives them, and the Python wrapper refuses
what is not a set of matching float32 device tensors before it calls the library.  The queries themselves are tested on the GPU
(tests/test_gpu_ray_query.py)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import raytracing_engine_amd as R
from raytracing_engine_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCTIONS = ("rt_default_ray_query_params", "rt_query_rays_device", "rt_get_ray_query_stats")


def test_the_functions_are_exported_and_bound():
    lib = R.load()
    for name in FUNCTIONS:
        assert hasattr(lib, name), name
        assert name in _lib.PROTOTYPES, name
    assert lib.rt_abi_version() == 4  # additions only


def test_a_null_context_is_refused():
    lib = R.load()
    p = R.RayQueryParams()
    assert lib.rt_query_rays_device(None, None, None, None, 0, None, None, None) == -1  # RT_ERR_INVALID: nothing touched
    assert lib.rt_query_rays_device(None, C.c_void_p(16), C.c_void_p(16), None, 1, C.byref(p), C.c_void_p(16), C.c_void_p(16)) == -1
    assert lib.rt_get_ray_query_stats(None, C.byref(R.RayQueryStats())) == -1
    assert lib.rt_default_ray_query_params(None) == -1


def test_struct_layouts_match_the_header(tmp_path):
    """sizeof/offsetof as gcc computes them from include/rt_abi.h vs the ctypes mirrors."""
    pf = [n for n, _ in R.RayQueryParams._fields_]
    sf = [n for n, _ in R.RayQueryStats._fields_]
    prog = tmp_path / "layout.c"
    prog.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"rt_abi.h\"\nint main(void) {\n"
                    "    printf(\"%zu %zu %d %d\\n\", sizeof(rt_ray_query_params), sizeof(rt_ray_query_stats), RT_RAY_MISS, RT_RAY_INVALID);\n"
                    + "".join(f"    printf(\"%zu\\n\", offsetof(rt_ray_query_params, {n}));\n" for n in pf)
                    + "".join(f"    printf(\"%zu\\n\", offsetof(rt_ray_query_stats, {n}));\n" for n in sf)
                    + "    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out[:4] == [C.sizeof(R.RayQueryParams), C.sizeof(R.RayQueryStats), _lib.RAY_MISS, _lib.RAY_INVALID]
    assert out[4:4 + len(pf)] == [getattr(R.RayQueryParams, n).offset for n in pf]
    assert out[4 + len(pf):] == [getattr(R.RayQueryStats, n).offset for n in sf]
    assert pf == ["any_hit", "tune_refill_min", "tune_blocks_per_cu", "tune_lds_stack", "tune_max_blocks"]
    assert sf == ["rays", "invalid_rays", "stack_overflow", "launches", "ms"]
    assert (R.Renderer.RAY_MISS, R.Renderer.RAY_INVALID) == (-1, -2)


def test_default_params_are_zeros():
    lib = R.load()
    p = R.RayQueryParams(7, 7, 7, 7, 7)
    assert lib.rt_default_ray_query_params(C.byref(p)) == 0
    assert bytes(p) == bytes(C.sizeof(R.RayQueryParams))


def test_the_wrapper_checks_its_tensors_before_the_library():
    torch = pytest.importorskip("torch")
    r = R.Renderer.__new__(R.Renderer)  # no context: every argument below must be refused before the library is called
    r._lib, r._ctx, r.device = None, None, 0
    a = np.zeros((4, 3), np.float32)
    good = torch.from_numpy(a)  # float32, contiguous, the right shape - but a CPU tensor
    bad_rays = dict(numpy=a, cpu=good, float64=good.double(), non_contiguous=torch.zeros(3, 4).t(), four_columns=torch.zeros(4, 4))
    for what, bad in bad_rays.items():
        with pytest.raises(ValueError):
            r.query_rays(bad, good)
        with pytest.raises(ValueError):
            r.query_rays(good, bad)
        with pytest.raises(ValueError):
            r.query_rays(bad, bad, any_hit=True)
    with pytest.raises(ValueError):
        r.query_rays(torch.zeros(4, 3), torch.zeros(5, 3))  # different lengths
    with pytest.raises(ValueError):
        r.query_rays(torch.zeros(4, 3), torch.zeros(4, 3), tmax=torch.zeros(3))  # a tmax of the wrong length
    with pytest.raises(ValueError):
        r.query_rays(torch.zeros(4, 3), torch.zeros(4, 3), tmax=np.zeros(4, np.float32))


def test_the_wrapper_compares_lengths_and_shapes():
    """The same refusals past the device check (a renderer that takes CPU tensors for its device's): lengths and shapes are compared by
    the wrapper itself, and unknown tuning names are refused."""
    torch = pytest.importorskip("torch")

    class OnCpu(R.Renderer):
        def _device_rows(self, t, name, width):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or not t.is_contiguous():
                raise ValueError(name)
            if t.dim() == 2 and t.shape[1] == width:
                return t.shape[0]
            if t.dim() == 1 and t.numel() % width == 0:
                return t.numel() // width
            raise ValueError(name)

    r = OnCpu.__new__(OnCpu)
    r._lib, r._ctx, r.device = None, None, 0
    o, d = torch.zeros(4, 3), torch.zeros(4, 3)
    with pytest.raises(ValueError, match="disagree"):
        r.query_rays(o, torch.zeros(5, 3))
    with pytest.raises(ValueError, match="disagree"):
        r.query_rays(o, torch.zeros(15))
    with pytest.raises(ValueError, match="origins"):
        r.query_rays(torch.zeros(4, 4), d)
    for bad_tmax in (torch.zeros(3), torch.zeros(5), torch.zeros(4, 1)):
        with pytest.raises(ValueError, match="tmax"):
            r.query_rays(o, d, tmax=bad_tmax)
    with pytest.raises(ValueError, match="out"):
        r.query_rays(o, d, out=torch.zeros(4))  # a closest-hit query fills a pair
    with pytest.raises(TypeError):
        r.query_rays(o, d, tune_nothing=1)
