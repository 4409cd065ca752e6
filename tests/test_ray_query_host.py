"""CPU tests of the ray-query boundary (rt_query_rays_device / Renderer.query_rays): the library exports and binds the three
functions, a NULL context is refused without a GPU, the two structs have the layout gcc gives them, and the Python wrapper refuses
what is not a set of matching float32 device tensors before it calls the library.  The queries themselves are tested on the GPU
(tests/test_gpu_ray_query.py)."""
import ctypes as C

import numpy as np
import pytest

import abi_boundary as AB
import raytracing_engine_amd as R
from raytracing_engine_amd import _lib

FUNCTIONS = ("rt_default_ray_query_params", "rt_query_rays_device", "rt_get_ray_query_stats")
V = C.c_void_p(16)
KIND = AB.Kind(functions=FUNCTIONS, params="RayQueryParams", stats="RayQueryStats", params_c="rt_ray_query_params", stats_c="rt_ray_query_stats",
               params_fields=["any_hit", "tune_refill_min", "tune_blocks_per_cu", "tune_lds_stack", "tune_max_blocks"],
               stats_fields=["rays", "invalid_rays", "stack_overflow", "launches", "ms"],
               constants={"RT_RAY_MISS": _lib.RAY_MISS, "RT_RAY_INVALID": _lib.RAY_INVALID}, default="rt_default_ray_query_params",
               null_calls=(("rt_query_rays_device", (None, None, None, 0, None, None, None)),
                           ("rt_query_rays_device", (V, V, None, 1, C.byref(R.RayQueryParams()), V, V)),
                           ("rt_get_ray_query_stats", (C.byref(R.RayQueryStats()),)), ("rt_default_ray_query_params", ())))


def test_the_functions_are_exported_and_bound():
    AB.exports(KIND)


def test_a_null_context_is_refused():
    AB.null_context(KIND)


def test_struct_layouts_match_the_header(tmp_path):
    """sizeof/offsetof as gcc computes them from include/rt_abi.h vs the ctypes mirrors."""
    AB.struct_layout(KIND, tmp_path)
    assert (R.Renderer.RAY_MISS, R.Renderer.RAY_INVALID) == (-1, -2)


def test_default_params_are_zeros():
    AB.default_params(KIND)


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

    r = AB.cpu_renderer()
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
